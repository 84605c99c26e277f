"""Synthetic structured hex meshes (SURVEY.md §8d generator).

Unit-spacing cube of n^3 C3D8 (HEC-MW TYPE=361) elements, (n+1)^3 nodes,
node id = 1 + i + (n+1)*(j + (n+1)*k), connectivity bottom face CCW then top
face.  Boundary conditions of the benchmark decks: all three dofs fixed on the
z=0 face, unit x-load on every z=n node.  Deterministic, no RNG.

All index arrays are int32 and 1-based, as in hecmwST_local_mesh
(hecmw_util_f.F90:232-381): ``elem_node_item`` is the flattened connectivity.
"""
import numpy as np


class CubeMesh:
    def __init__(self, n, spacing=1.0, skew=0.0):
        """n elements per edge.  ``skew`` > 0 perturbs interior nodes
        deterministically (to exercise non-trivial Jacobians in tests)."""
        self.n = int(n)
        m = self.n + 1
        self.n_node = m ** 3
        self.n_elem = self.n ** 3
        k, j, i = np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij")
        xyz = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.float64) * spacing
        if skew:
            nid = np.arange(self.n_node, dtype=np.float64)
            interior = ((i > 0) & (i < self.n) & (j > 0) & (j < self.n) & (k > 0) & (k < self.n)).ravel()
            d = np.stack([np.sin(1.3 * nid + 0.1), np.sin(2.1 * nid + 0.7), np.sin(0.7 * nid + 1.9)], axis=1)
            xyz[interior] += skew * spacing * d[interior]
        self.coord = np.ascontiguousarray(xyz)                 # (n_node, 3)
        ek, ej, ei = np.meshgrid(np.arange(self.n), np.arange(self.n), np.arange(self.n), indexing="ij")
        n0 = (1 + ei + m * (ej + m * ek)).ravel()
        conn = np.stack([n0, n0 + 1, n0 + 1 + m, n0 + m,
                         n0 + m * m, n0 + 1 + m * m, n0 + 1 + m + m * m, n0 + m + m * m], axis=1)
        self.conn = np.ascontiguousarray(conn.astype(np.int32))  # (n_elem, 8), 1-based
        self.bottom_nodes = (1 + np.arange(m * m)).astype(np.int32)
        self.top_nodes = (1 + self.n * m * m + np.arange(m * m)).astype(np.int32)

    @property
    def ndof(self):
        return 3 * self.n_node

    def dirichlet(self):
        """(node, dof, value) triplets: z=0 face clamped."""
        node = np.repeat(self.bottom_nodes, 3).astype(np.int32)
        dof = np.tile(np.array([1, 2, 3], dtype=np.int32), self.bottom_nodes.size)
        val = np.zeros(node.size, dtype=np.float64)
        return node, dof, val

    def load(self):
        """!CLOAD 1.0 in x on every z=n node."""
        b = np.zeros(3 * self.n_node, dtype=np.float64)
        b[3 * (self.top_nodes - 1)] = 1.0
        return b


def cube_blocks(n):
    """Closed-form block counts of the n-element cube: (N, NPL, NPU, nb)."""
    m = n + 1
    N = m ** 3
    nb = (3 * m - 2) ** 3
    return N, (nb - N) // 2, (nb - N) // 2, nb


class PieMesh:
    """Solid cylinder of radius ``radius`` and height ``height`` meshed the way a hex-only mesher meshes a solid of
    revolution: ``n_r`` rings of ``n_theta`` sectors on ``n_z`` layers, the innermost ring collapsed onto the axis.
    Each layer has one axis node; ring node (ir, it) sits at radius radius * ir / n_r, angle 2 pi it / n_theta.
    Element (ir, it) has the corners [(ir, it), (ir+1, it), (ir+1, it+1), (ir, it+1)], bottom face then top (positive
    Jacobians); for ir = 0 nodes 0 and 3 (and 4 and 7) are the same axis node: a collapsed hexahedron naming a node
    twice.  ``sectors`` < n_theta keeps only the first sectors columns (an open wedge; sectors=1, n_r=1, n_z=1 is a
    single collapsed element).  Elements are numbered layer by layer, ring by ring, sector by sector.  Deterministic."""

    def __init__(self, n_theta, n_r, n_z, radius=1.0, height=1.0, sectors=None):
        self.n_theta, self.n_r, self.n_z = int(n_theta), int(n_r), int(n_z)
        ns = self.n_theta if sectors is None else int(sectors)
        closed = ns == self.n_theta
        ncol = ns if closed else ns + 1              # ring node columns per ring
        per_layer = 1 + self.n_r * ncol
        self.n_node = per_layer * (self.n_z + 1)
        xyz = np.zeros((self.n_node, 3))
        for k in range(self.n_z + 1):
            base = k * per_layer
            xyz[base] = (0.0, 0.0, height * k / self.n_z)
            for ir in range(1, self.n_r + 1):
                for it in range(ncol):
                    ang = 2.0 * np.pi * it / self.n_theta
                    r = radius * ir / self.n_r
                    xyz[base + 1 + (ir - 1) * ncol + it] = (r * np.cos(ang), r * np.sin(ang), height * k / self.n_z)
        self.coord = np.ascontiguousarray(xyz)

        def nid(k, ir, it):                          # 1-based
            if ir == 0:
                return 1 + k * per_layer
            return 1 + k * per_layer + 1 + (ir - 1) * ncol + (it % ncol if closed else it)
        conn = []
        for k in range(self.n_z):
            for ir in range(self.n_r):
                for it in range(ns):
                    face = [(ir, it), (ir + 1, it), (ir + 1, it + 1), (ir, it + 1)]
                    conn.append([nid(k, *p) for p in face] + [nid(k + 1, *p) for p in face])
        self.conn = np.ascontiguousarray(np.array(conn, dtype=np.int32))
        self.n_elem = self.conn.shape[0]
        self.bottom_nodes = (1 + np.arange(per_layer)).astype(np.int32)
        self.top_nodes = (1 + self.n_z * per_layer + np.arange(per_layer)).astype(np.int32)
        self.axis_nodes = (1 + per_layer * np.arange(self.n_z + 1)).astype(np.int32)

    @property
    def ndof(self):
        return 3 * self.n_node

    def dirichlet(self):
        """(node, dof, value) triplets: z=0 face clamped."""
        node = np.repeat(self.bottom_nodes, 3).astype(np.int32)
        dof = np.tile(np.array([1, 2, 3], dtype=np.int32), self.bottom_nodes.size)
        return node, dof, np.zeros(node.size, dtype=np.float64)

    def load(self):
        """Unit x-load on every node of the top face."""
        b = np.zeros(3 * self.n_node, dtype=np.float64)
        b[3 * (self.top_nodes - 1)] = 1.0
        return b


class RenumberedMesh:
    """``mesh`` with its node ids and its element order permuted at random (``renumber``).  Coordinates, connectivity,
    boundary conditions, load and the node sets a mesh names (bottom / top / axis nodes) follow the new numbering."""

    def __init__(self, mesh, seed):
        rng = np.random.default_rng(seed)
        self.base = mesh
        self.n_node, self.n_elem = mesh.n_node, mesh.conn.shape[0]
        self.new_of_old = (1 + rng.permutation(self.n_node)).astype(np.int32)   # old id - 1 -> new id
        self.elem_order = rng.permutation(self.n_elem)                          # new element -> old element
        old_of_new = np.empty(self.n_node, dtype=np.int64)
        old_of_new[self.new_of_old - 1] = np.arange(self.n_node)
        self.coord = np.ascontiguousarray(mesh.coord[old_of_new])
        self.conn = np.ascontiguousarray(self.new_of_old[mesh.conn[self.elem_order] - 1].astype(np.int32))
        for name in ("bottom_nodes", "top_nodes", "axis_nodes"):
            if hasattr(mesh, name):
                setattr(self, name, self.new_of_old[getattr(mesh, name) - 1])

    @property
    def ndof(self):
        return 3 * self.n_node

    def dirichlet(self):
        node, dof, val = self.base.dirichlet()
        return self.new_of_old[node - 1].astype(np.int32), dof, val

    def load(self):
        return self.renumber_field(self.base.load())

    def renumber_field(self, f):
        """A nodal field (3 values per node) of the base mesh in the new numbering."""
        out = np.empty_like(f)
        out.reshape(-1, 3)[self.new_of_old - 1] = f.reshape(-1, 3)
        return out


def renumber(mesh, seed):
    """Random permutation of the node ids and of the element order of ``mesh`` (np.random.default_rng(seed))."""
    return RenumberedMesh(mesh, seed)


def color_elements(conn, n_node):
    """Python restatement of the host's greedy element colouring (fx_order.cpp color_elements): each element takes the
    lowest of 64 colours no element sharing a node holds.  Returns the colour per element, or None when some element
    finds all 64 taken (the library then scatters with atomics)."""
    used = np.zeros(n_node + 1, dtype=np.uint64)
    col = np.zeros(conn.shape[0], dtype=np.int32)
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    for e, nodes in enumerate(conn):
        m = np.uint64(0)
        for v in nodes:
            m |= used[v]
        if m == full:
            return None
        free = int(~m & full)
        c = (free & -free).bit_length() - 1
        col[e] = c
        for v in nodes:
            used[v] |= np.uint64(1) << np.uint64(c)
    return col


# Kuhn split of a hexahedron into 6 tetrahedra: every tetrahedron runs from corner (0,0,0) to corner (1,1,1) of the cube along
# one permutation of the axes.  All cubes use the same diagonal, so neighbouring faces are split the same way (the mesh is
# conforming).  Positions in CubeMesh's connectivity (bottom face counter-clockwise, then top); each tetrahedron is ordered for
# a positive volume.
_KUHN = ((0, 1, 2, 6), (0, 5, 1, 6), (0, 2, 3, 6), (0, 3, 7, 6), (0, 4, 5, 6), (0, 7, 4, 6))
# mid-edge nodes of the 10-node tetrahedron (HEC-MW TYPE=342, FrontISTR order): 5=(1,2), 6=(2,3), 7=(3,1), 8=(1,4), 9=(2,4), 10=(3,4)
TET10_EDGES = ((0, 1), (1, 2), (2, 0), (0, 3), (1, 3), (2, 3))


class TetMesh:
    """The n^3 cube of CubeMesh with every hexahedron split into 6 tetrahedra (Kuhn split, conforming): TYPE=341 (4 nodes) or,
    with one node added at the middle of every edge, TYPE=342 (10 nodes, FrontISTR's node order).  The vertices keep CubeMesh's
    numbering; the mid-edge nodes follow, in the order of their edges sorted by (lower, higher) vertex id.  ``skew`` moves the
    interior vertices as CubeMesh does; ``curve`` then moves the interior mid-edge nodes off their edges (curved 342 elements).
    Boundary conditions and load as CubeMesh: the z=0 face clamped, unit x-load on every node of the z=n face."""

    def __init__(self, n, etype=342, spacing=1.0, skew=0.0, curve=0.0):
        if etype not in (341, 342):
            raise ValueError("etype must be 341 or 342")
        hexes = CubeMesh(n, spacing=spacing, skew=skew)
        self.n, self.etype = int(n), int(etype)
        tets = np.concatenate([hexes.conn[:, list(t)] for t in _KUHN], axis=1).reshape(-1, 4)  # hex by hex, 6 each
        coord = hexes.coord
        if etype == 342:
            pairs = np.stack([tets[:, list(e)] for e in TET10_EDGES], axis=1)        # (n_tet, 6, 2)
            key = np.sort(pairs, axis=2).reshape(-1, 2)
            edges, inverse = np.unique(key, axis=0, return_inverse=True)
            mid = 0.5 * (coord[edges[:, 0] - 1] + coord[edges[:, 1] - 1])
            if curve:
                eid = np.arange(edges.shape[0], dtype=np.float64)
                lo, hi = 0.0, self.n * spacing
                inside = np.all((mid > lo + 1e-9 * spacing) & (mid < hi - 1e-9 * spacing), axis=1)
                d = np.stack([np.sin(0.9 * eid + 0.3), np.sin(1.7 * eid + 1.1), np.sin(2.3 * eid + 0.5)], axis=1)
                mid[inside] += curve * spacing * d[inside]
            tets = np.concatenate([tets, hexes.n_node + 1 + inverse.reshape(-1, 6)], axis=1)
            coord = np.concatenate([coord, mid])
        self.coord = np.ascontiguousarray(coord)
        self.conn = np.ascontiguousarray(tets.astype(np.int32))
        self.n_node, self.n_elem = self.coord.shape[0], self.conn.shape[0]
        z = self.coord[:, 2]
        self.bottom_nodes = (1 + np.flatnonzero(z == 0.0)).astype(np.int32)
        self.top_nodes = (1 + np.flatnonzero(z == self.n * spacing)).astype(np.int32)

    @property
    def ndof(self):
        return 3 * self.n_node

    def dirichlet(self):
        """(node, dof, value) triplets: z=0 face clamped."""
        node = np.repeat(self.bottom_nodes, 3).astype(np.int32)
        dof = np.tile(np.array([1, 2, 3], dtype=np.int32), self.bottom_nodes.size)
        return node, dof, np.zeros(node.size, dtype=np.float64)

    def load(self):
        """1.0 in x on every node of the z=n face."""
        b = np.zeros(3 * self.n_node, dtype=np.float64)
        b[3 * (self.top_nodes - 1)] = 1.0
        return b


# Wedges and the 20-node hexahedron (HEC-MW TYPE=351, 352, 362; FrontISTR's node order).  A hexahedron of CubeMesh (bottom
# face counter-clockwise 0-3, top face 4-7) splits along the diagonal 0-2 of its bottom and top faces into two prisms, each
# listed bottom triangle (counter-clockwise seen from above) then top triangle; every cube uses the same diagonal and the
# vertical faces stay whole, so the mesh is conforming.
_PRISMS = ((0, 1, 2, 4, 5, 6), (0, 2, 3, 4, 6, 7))
# mid-edge nodes of the 15-node prism: 7-9 bottom triangle (1,2), (2,3), (3,1); 10-12 top triangle (4,5), (5,6), (6,4); 13-15
# the vertical edges (1,4), (2,5), (3,6)
PRISM15_EDGES = ((0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (0, 3), (1, 4), (2, 5))
# mid-edge nodes of the 20-node hexahedron: 9-12 bottom face (1,2), (2,3), (3,4), (4,1); 13-16 top face (5,6), (6,7), (7,8),
# (8,5); 17-20 the vertical edges (1,5), (2,6), (3,7), (4,8)
HEX20_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
C3_NODES = {341: 4, 342: 10, 351: 6, 352: 15, 361: 8, 362: 20}
C3_POINTS = {341: 1, 342: 4, 351: 2, 352: 9, 361: 8, 362: 27}          # NumOfQuadPoints
C3_EDGES = {342: TET10_EDGES, 352: PRISM15_EDGES, 362: HEX20_EDGES}
# getSubFace (fistr1/src/lib/element/element.f90:181-315): the nodes of face f, 1-based positions in the element
C3_SUBFACE = {
    341: ((1, 2, 3), (4, 2, 1), (4, 3, 2), (4, 1, 3)),
    342: ((1, 2, 3, 5, 6, 7), (4, 2, 1, 9, 5, 8), (4, 3, 2, 10, 6, 9), (4, 1, 3, 8, 7, 10)),
    351: ((1, 2, 3), (6, 5, 4), (4, 5, 2, 1), (5, 6, 3, 2), (6, 4, 1, 3)),
    352: ((1, 2, 3, 7, 8, 9), (6, 5, 4, 11, 10, 12), (4, 5, 2, 1, 10, 14, 7, 13), (5, 6, 3, 2, 11, 15, 8, 14),
          (6, 4, 1, 3, 12, 13, 9, 15)),
    361: ((1, 2, 3, 4), (8, 7, 6, 5), (5, 6, 2, 1), (6, 7, 3, 2), (7, 8, 4, 3), (8, 5, 1, 4)),
    362: ((1, 2, 3, 4, 9, 10, 11, 12), (8, 7, 6, 5, 15, 14, 13, 16), (5, 6, 2, 1, 13, 18, 9, 17),
          (6, 7, 3, 2, 14, 19, 10, 18), (7, 8, 4, 3, 15, 20, 11, 19), (8, 5, 1, 4, 16, 17, 12, 20)),
}


def _add_midedge_nodes(coord, conn, edges, curve, lo, hi, spacing):
    """One node at the middle of every edge of the first-order elements ``conn``: appended after the vertices in the order of
    the edges sorted by (lower, higher) vertex id; ``curve`` moves the interior ones off their edges."""
    pairs = np.stack([conn[:, list(e)] for e in edges], axis=1)
    key = np.sort(pairs, axis=2).reshape(-1, 2)
    uniq, inverse = np.unique(key, axis=0, return_inverse=True)
    mid = 0.5 * (coord[uniq[:, 0] - 1] + coord[uniq[:, 1] - 1])
    if curve:
        eid = np.arange(uniq.shape[0], dtype=np.float64)
        inside = np.all((mid > lo + 1e-9 * spacing) & (mid < hi - 1e-9 * spacing), axis=1)
        d = np.stack([np.sin(0.9 * eid + 0.3), np.sin(1.7 * eid + 1.1), np.sin(2.3 * eid + 0.5)], axis=1)
        mid[inside] += curve * spacing * d[inside]
    conn = np.concatenate([conn, coord.shape[0] + 1 + inverse.reshape(-1, len(edges))], axis=1)
    return np.concatenate([coord, mid]), conn


class _CubeOfSolids:
    """Common part of WedgeMesh and Hex20Mesh: boundary sets by coordinate, the clamp and the load of CubeMesh."""

    def _finish(self, coord, conn, n, spacing):
        self.coord = np.ascontiguousarray(coord)
        self.conn = np.ascontiguousarray(conn.astype(np.int32))
        self.n_node, self.n_elem = self.coord.shape[0], self.conn.shape[0]
        z = self.coord[:, 2]
        self.bottom_nodes = (1 + np.flatnonzero(z == 0.0)).astype(np.int32)
        self.top_nodes = (1 + np.flatnonzero(z == n * spacing)).astype(np.int32)

    @property
    def ndof(self):
        return 3 * self.n_node

    def dirichlet(self):
        """(node, dof, value) triplets: z=0 face clamped."""
        node = np.repeat(self.bottom_nodes, 3).astype(np.int32)
        dof = np.tile(np.array([1, 2, 3], dtype=np.int32), self.bottom_nodes.size)
        return node, dof, np.zeros(node.size, dtype=np.float64)

    def load(self):
        """1.0 in x on every node of the z=n face."""
        b = np.zeros(3 * self.n_node, dtype=np.float64)
        b[3 * (self.top_nodes - 1)] = 1.0
        return b


class WedgeMesh(_CubeOfSolids):
    """The n^3 cube of CubeMesh with every hexahedron split into 2 prisms: TYPE=351 (6 nodes) or, with one node added at the
    middle of every edge, TYPE=352 (15 nodes).  Vertex numbering, ``skew``, ``curve``, boundary conditions and load as
    TetMesh."""

    def __init__(self, n, etype=352, spacing=1.0, skew=0.0, curve=0.0):
        if etype not in (351, 352):
            raise ValueError("etype must be 351 or 352")
        hexes = CubeMesh(n, spacing=spacing, skew=skew)
        self.n, self.etype = int(n), int(etype)
        conn = np.concatenate([hexes.conn[:, list(p)] for p in _PRISMS], axis=1).reshape(-1, 6)   # hex by hex, 2 each
        coord = hexes.coord
        if etype == 352:
            coord, conn = _add_midedge_nodes(coord, conn, PRISM15_EDGES, curve, 0.0, self.n * spacing, spacing)
        self._finish(coord, conn, self.n, spacing)


class Hex20Mesh(_CubeOfSolids):
    """The n^3 cube of CubeMesh as TYPE=362 elements: one node added at the middle of every edge (20 nodes per element)."""

    def __init__(self, n, spacing=1.0, skew=0.0, curve=0.0):
        hexes = CubeMesh(n, spacing=spacing, skew=skew)
        self.n, self.etype = int(n), 362
        coord, conn = _add_midedge_nodes(hexes.coord, hexes.conn, HEX20_EDGES, curve, 0.0, self.n * spacing, spacing)
        self._finish(coord, conn, self.n, spacing)


def solid_mesh(n, etype, **kw):
    """The cube of n^3 cells as elements of ``etype``: 341 / 342 TetMesh, 351 / 352 WedgeMesh, 362 Hex20Mesh."""
    if etype in (341, 342):
        return TetMesh(n, etype=etype, **kw)
    if etype in (351, 352):
        return WedgeMesh(n, etype=etype, **kw)
    if etype == 362:
        return Hex20Mesh(n, **kw)
    raise ValueError("etype must be 341, 342, 351, 352 or 362")


# A hexahedron of CubeMesh split into 2 prisms whose axis runs along x: the triangles lie in the x = const faces, cut along the
# diagonal from their (low y, low z) corner to their (high y, high z) corner -- the diagonal the Kuhn split puts on that face --
# each listed x = low triangle (counter-clockwise seen from +x) then x = high triangle.  The y and z faces stay whole.
_PRISMS_X = ((0, 3, 7, 1, 2, 6), (0, 7, 4, 1, 6, 5))


def _add_midedge_nodes_groups(coord, conns, edge_tables, curve, lo, hi, spacing):
    """_add_midedge_nodes for several first-order connectivities at once: one node per edge of the whole mesh, shared by
    every element (of whatever type) that holds the edge; numbered after the vertices in the order of the edges sorted by
    (lower, higher) vertex id."""
    keys = [np.sort(np.stack([c[:, list(e)] for e in edges], axis=1), axis=2).reshape(-1, 2)
            for c, edges in zip(conns, edge_tables)]
    uniq, inverse = np.unique(np.concatenate(keys), axis=0, return_inverse=True)
    inverse = inverse.ravel()
    mid = 0.5 * (coord[uniq[:, 0] - 1] + coord[uniq[:, 1] - 1])
    if curve:
        eid = np.arange(uniq.shape[0], dtype=np.float64)
        inside = np.all((mid > lo + 1e-9 * spacing) & (mid < hi - 1e-9 * spacing), axis=1)
        d = np.stack([np.sin(0.9 * eid + 0.3), np.sin(1.7 * eid + 1.1), np.sin(2.3 * eid + 0.5)], axis=1)
        mid[inside] += curve * spacing * d[inside]
    out, at = [], 0
    for c, edges, k in zip(conns, edge_tables, keys):
        out.append(np.concatenate([c, coord.shape[0] + 1 + inverse[at:at + k.shape[0]].reshape(-1, len(edges))], axis=1))
        at += k.shape[0]
    return np.concatenate([coord, mid]), out


class MixedMesh(_CubeOfSolids):
    """A conforming cube of three solid element types: the pattern of the reference's examples/static/refine/hexpritet sample,
    extruded along y.  The n^3 cells of CubeMesh (n >= 2) are split at h = n // 2 in x and z.  Looking at the (x, z) plane:

        low x,  low z   hexahedra                                        TYPE=361 (order 1) / 362 (order 2)
        high x, low z   2 wedges per cell, axis along z (_PRISMS)        TYPE=351 / 352
        low x,  high z  2 wedges per cell, axis along x (_PRISMS_X)      TYPE=351 / 352
        high x, high z  6 tetrahedra per cell (Kuhn split)               TYPE=341 / 342

    The hexahedra meet both wedge quadrants in whole quadrilaterals; the tetrahedra meet the z-axis wedges in the z = h
    triangles and the x-axis wedges in the x = h triangles, both cut along the diagonal the Kuhn split uses.  ``order=2`` adds
    one node at the middle of every edge of the mesh, shared across the types.  ``groups``: [(etype, conn, elemopt, elem_mat)]
    in mesh order (hexahedra, wedges -- the z-axis quadrant first --, tetrahedra), the argument of
    SolverContext.assemble_groups; ``elem_offsets``: first element of each group (+ end) in that order.  ``skew``, ``curve``,
    boundary conditions and load as the single-type builders."""

    def __init__(self, n, order=1, spacing=1.0, skew=0.0, curve=0.0):
        if order not in (1, 2):
            raise ValueError("order must be 1 or 2")
        if n < 2:
            raise ValueError("n must be >= 2")
        hexes = CubeMesh(n, spacing=spacing, skew=skew)
        self.n, self.order = int(n), int(order)
        h = self.n // 2
        ek, ej, ei = np.meshgrid(np.arange(self.n), np.arange(self.n), np.arange(self.n), indexing="ij")
        ei, ek = ei.ravel(), ek.ravel()
        cells = hexes.conn
        hex_c = cells[(ei < h) & (ek < h)]
        wz = np.concatenate([cells[(ei >= h) & (ek < h)][:, list(p)] for p in _PRISMS], axis=1).reshape(-1, 6)
        wx = np.concatenate([cells[(ei < h) & (ek >= h)][:, list(p)] for p in _PRISMS_X], axis=1).reshape(-1, 6)
        tet = np.concatenate([cells[(ei >= h) & (ek >= h)][:, list(t)] for t in _KUHN], axis=1).reshape(-1, 4)
        conns = [hex_c, np.concatenate([wz, wx]), tet]
        coord = hexes.coord
        self.etypes = (361, 351, 341) if order == 1 else (362, 352, 342)
        if order == 2:
            coord, conns = _add_midedge_nodes_groups(coord, conns, (HEX20_EDGES, PRISM15_EDGES, TET10_EDGES), curve, 0.0,
                                                     self.n * spacing, spacing)
        self.conns = [np.ascontiguousarray(c.astype(np.int32)) for c in conns]
        self.coord = np.ascontiguousarray(coord)
        self.n_node = self.coord.shape[0]
        self.elem_offsets = np.concatenate([[0], np.cumsum([c.shape[0] for c in self.conns])]).astype(np.int64)
        self.n_elem = int(self.elem_offsets[-1])
        z = self.coord[:, 2]
        self.bottom_nodes = (1 + np.flatnonzero(z == 0.0)).astype(np.int32)
        self.top_nodes = (1 + np.flatnonzero(z == self.n * spacing)).astype(np.int32)

    def groups_with(self, elemopt=1, elem_mat=None):
        """The groups with ``elemopt`` for the 361 group and the per-element material ids ``elem_mat`` (1-based, mesh order)
        cut into the groups."""
        o = self.elem_offsets
        return [(et, c, elemopt, None if elem_mat is None else np.ascontiguousarray(elem_mat[o[g]:o[g + 1]], dtype=np.int32))
                for g, (et, c) in enumerate(zip(self.etypes, self.conns))]

    @property
    def groups(self):
        return self.groups_with()


def mesh_groups(mesh, elemopt=1, elem_mat=None):
    """[(etype, conn, elemopt, elem_mat)] of any mesh of this module, the ``groups`` argument of SolverContext.assemble_groups,
    update_groups_linear and thermal_load_groups: MixedMesh / RenumberedGroups give their own, a single-type mesh gives one
    group (CubeMesh, PieMesh: TYPE=361; the others their ``etype``).  elem_mat: 1-based material id per element, mesh order."""
    if hasattr(mesh, "groups_with"):
        return mesh.groups_with(elemopt, elem_mat)
    em = None if elem_mat is None else np.ascontiguousarray(elem_mat, dtype=np.int32)
    return [(int(getattr(mesh, "etype", 361)), mesh.conn, elemopt, em)]


class RenumberedGroups:
    """A mesh of element groups (MixedMesh) with its node ids permuted at random and the elements of every group shuffled
    within the group (np.random.default_rng(seed)); what RenumberedMesh is to the single-type builders."""

    def __init__(self, mesh, seed):
        rng = np.random.default_rng(seed)
        self.base = mesh
        self.n_node, self.n_elem = mesh.n_node, mesh.n_elem
        self.etypes, self.elem_offsets = mesh.etypes, mesh.elem_offsets
        self.new_of_old = (1 + rng.permutation(self.n_node)).astype(np.int32)
        old_of_new = np.empty(self.n_node, dtype=np.int64)
        old_of_new[self.new_of_old - 1] = np.arange(self.n_node)
        self.coord = np.ascontiguousarray(mesh.coord[old_of_new])
        self.elem_orders = [rng.permutation(c.shape[0]) for c in mesh.conns]     # per group: new element -> old element
        self.conns = [np.ascontiguousarray(self.new_of_old[c[o] - 1].astype(np.int32)) for c, o in zip(mesh.conns, self.elem_orders)]
        self.bottom_nodes = self.new_of_old[mesh.bottom_nodes - 1]
        self.top_nodes = self.new_of_old[mesh.top_nodes - 1]

    ndof = property(lambda self: 3 * self.n_node)
    groups = property(lambda self: self.groups_with())

    def groups_with(self, elemopt=1, elem_mat=None):
        """``elem_mat`` in the BASE mesh's element order; it follows the shuffled elements."""
        o = self.elem_offsets
        return [(et, c, elemopt, None if elem_mat is None else
                 np.ascontiguousarray(np.asarray(elem_mat)[o[g]:o[g + 1]][self.elem_orders[g]], dtype=np.int32))
                for g, (et, c) in enumerate(zip(self.etypes, self.conns))]

    def dirichlet(self):
        node, dof, val = self.base.dirichlet()
        return self.new_of_old[node - 1].astype(np.int32), dof, val

    def load(self):
        f = self.base.load()
        out = np.empty_like(f)
        out.reshape(-1, 3)[self.new_of_old - 1] = f.reshape(-1, 3)
        return out


def renumber_groups(mesh, seed):
    """renumber() for a mesh of element groups."""
    return RenumberedGroups(mesh, seed)
