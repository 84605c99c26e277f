"""Synthetic block systems with NDOF = 1, 2, 4, 6 (the reference's 11 / 22 / 44 / 66 / nn code paths) on the
profile of a skewed cube of hex8 elements: every element contributes a random SPD local matrix (seeded), node-major with
NDOF rows per node, so the global matrix is SPD with the reference's D / AL / AU layout (row-major NDOF x NDOF blocks).
nn_system is the small cube the stored answers were made on; cube_system builds the same thing vectorised at any size;
random_system is a profile that does not come from a mesh."""
import numpy as np

NN_NDOF = [1, 2, 4, 5, 6]
# (METHOD, PRECOND): CG / BiCGSTAB x SSOR (RCM + multicolour, the reference's OpenMP path) / DIAG
NN_CASES = [(1, 1), (1, 3), (2, 1), (2, 3)]


def nn_tag(nd, meth, pc):
    return "n%d_m%d_p%d_" % (nd, meth, pc)


def nn_system(ndof, m=4, seed=0, halo=0):
    from frontistr_amd.mesh import CubeMesh
    from oracle import pyoracle
    from oracle.refrun import BSR
    mesh = CubeMesh(m, skew=0.1)
    NP = mesh.n_node
    indexL, itemL, indexU, itemU = pyoracle.mat_con(NP, mesh.conn)
    nd2 = ndof * ndof
    D = np.zeros((NP, ndof, ndof))
    AL = np.zeros((itemL.size, ndof, ndof))
    AU = np.zeros((itemU.size, ndof, ndof))
    posL = {(i, int(itemL[j]) - 1): j for i in range(NP) for j in range(indexL[i], indexL[i + 1])}
    posU = {(i, int(itemU[j]) - 1): j for i in range(NP) for j in range(indexU[i], indexU[i + 1])}
    rng = np.random.default_rng(1000 * ndof + seed)
    for e in range(mesh.conn.shape[0]):
        nod = mesh.conn[e] - 1
        G = rng.standard_normal((8 * ndof, 8 * ndof))
        L = G @ G.T / (8 * ndof) + 0.02 * np.eye(8 * ndof)
        for a in range(8):
            for b in range(8):
                blk = L[a * ndof:(a + 1) * ndof, b * ndof:(b + 1) * ndof]
                i, j = int(nod[a]), int(nod[b])
                if i == j:
                    D[i] += blk
                elif j < i:
                    AL[posL[(i, j)]] += blk
                else:
                    AU[posU[(i, j)]] += blk
    B = rng.standard_normal(ndof * NP)
    A = BSR(NP, NP, indexL, itemL, indexU, itemU, D.ravel(), AL.ravel(), AU.ravel(), B, NDOF=ndof)
    return A


def cube_system(ndof, m, seed=0, halo=0, chunk=16384):
    """nn_system on m^3 elements, vectorised: the same random element matrices in the same order (nn_system(nd) ==
    cube_system(nd, 4) bit for bit), summed with np.add.at.  halo > 0: the last `halo` nodes are external (N = NP - halo)."""
    from frontistr_amd.mesh import CubeMesh
    from oracle import pyoracle
    from oracle.refrun import BSR
    mesh = CubeMesh(m, skew=0.1)
    NP = mesh.n_node
    indexL, itemL, indexU, itemU = pyoracle.mat_con(NP, mesh.conn)
    keyL = np.repeat(np.arange(NP, dtype=np.int64), np.diff(indexL)) * NP + (itemL - 1)
    keyU = np.repeat(np.arange(NP, dtype=np.int64), np.diff(indexU)) * NP + (itemU - 1)
    D = np.zeros((NP, ndof, ndof))
    AL = np.zeros((itemL.size, ndof, ndof))
    AU = np.zeros((itemU.size, ndof, ndof))
    rng = np.random.default_rng(1000 * ndof + seed)
    conn = mesh.conn.astype(np.int64) - 1
    n8 = 8 * ndof
    shift = 0.02 * np.eye(n8)
    for e0 in range(0, conn.shape[0], chunk):
        nod = conn[e0:e0 + chunk]
        c = nod.shape[0]
        G = rng.standard_normal((c, n8, n8))
        L = np.matmul(G, G.transpose(0, 2, 1)) / n8 + shift
        blk = L.reshape(c, 8, ndof, 8, ndof).transpose(0, 1, 3, 2, 4).reshape(-1, ndof, ndof)   # (element, a, b) order
        i = np.repeat(nod, 8, axis=1).ravel()
        j = np.tile(nod, (1, 8)).ravel()
        d, lo, up = i == j, j < i, j > i
        np.add.at(D, i[d], blk[d])
        np.add.at(AL, np.searchsorted(keyL, i[lo] * NP + j[lo]), blk[lo])
        np.add.at(AU, np.searchsorted(keyU, i[up] * NP + j[up]), blk[up])
    B = rng.standard_normal(ndof * NP)
    return BSR(NP - halo, NP, indexL, itemL, indexU, itemU, D.ravel(), AL.ravel(), AU.ravel(), B, NDOF=ndof)


def random_system(nd, N, n_halo, seed, hub=True, general=False):
    """Random symmetric profile with isolated nodes (rows holding only their diagonal block), hub rows, very uneven row lengths
    and halo columns.  hub: True = one hub row of up to 60 off-diagonal blocks; a sequence of sizes = one hub row per entry.
    Values: a 0.05 diagonal shift plus, per edge, [[P, -P], [-P, P]] with P SPD (symmetric blocks); general=True puts a random
    SPD 2*nd x 2*nd matrix on every edge instead, so the off-diagonal blocks are not symmetric (same profile)."""
    from oracle.refrun import BSR
    rng = np.random.default_rng(seed)
    NP = N + n_halo
    edges = set()
    live = np.arange(N)
    iso = set(rng.choice(N, 5, replace=False).tolist())
    live = np.array([i for i in live if i not in iso])
    for _ in range(3 * N):
        i, j = rng.choice(live, 2, replace=False)
        edges.add((min(i, j), max(i, j)))
    sizes = (60,) if hub is True else tuple(hub or ())
    for k, size in enumerate(sizes):
        h = int(live[(k + 1) * len(live) // (len(sizes) + 1)])
        for j in rng.choice(live, min(size, len(live) - 1), replace=False):
            if j != h:
                edges.add((min(h, int(j)), max(h, int(j))))
    for k in range(n_halo):                     # each halo node hangs on two internal rows
        for i in rng.choice(live, 2, replace=False):
            edges.add((int(i), N + k))
    low = [[] for _ in range(NP)]
    up = [[] for _ in range(NP)]
    for i, j in edges:
        up[i].append(j)
        if j < N:
            low[j].append(i)
    indexL, indexU = np.zeros(NP + 1, dtype=np.int32), np.zeros(NP + 1, dtype=np.int32)
    itemL, itemU = [], []
    for i in range(NP):
        low[i].sort(); up[i].sort()
        itemL += [c + 1 for c in low[i]]
        itemU += [c + 1 for c in up[i]]
        indexL[i + 1], indexU[i + 1] = len(itemL), len(itemU)
    posL = {(i, c): indexL[i] + k for i in range(NP) for k, c in enumerate(low[i])}
    posU = {(i, c): indexU[i] + k for i in range(NP) for k, c in enumerate(up[i])}
    D = np.tile(0.05 * np.eye(nd), (NP, 1, 1))
    AL = np.zeros((max(len(itemL), 1), nd, nd))
    AU = np.zeros((max(len(itemU), 1), nd, nd))
    for i, j in sorted(edges):
        if general:
            G = rng.standard_normal((2 * nd, 2 * nd))
            E = G @ G.T / (2 * nd) + 0.1 * np.eye(2 * nd)
            Pi, Pj, Pij, Pji = E[:nd, :nd], E[nd:, nd:], E[:nd, nd:], E[nd:, :nd]
        else:
            G = rng.standard_normal((nd, nd))
            P = G @ G.T / nd + 0.1 * np.eye(nd)
            Pi, Pj, Pij, Pji = P, P, -P, -P
        D[i] += Pi
        AU[posU[(i, j)]] = Pij
        if j < N:
            D[j] += Pj
            AL[posL[(j, i)]] = Pji
    B = rng.standard_normal(nd * NP)
    B[nd * N:] = 0.0
    A = BSR(N, NP, indexL, np.array(itemL, dtype=np.int32), indexU, np.array(itemU, dtype=np.int32), D.ravel(),
            AL[:len(itemL)].ravel(), AU[:len(itemU)].ravel(), B, NDOF=nd)
    return A


def wide_system(nd, n=160, seed=3):
    """Random symmetric block profile with some rows of more than 32 blocks (the one-thread-per-row factor kernel)."""
    from oracle.refrun import BSR
    rng = np.random.default_rng(seed)
    low = [set() for _ in range(n)]
    for i in range(n):
        for j in rng.choice(n, size=40 if i % 11 == 0 else 5, replace=False):
            if j != i:
                low[max(i, j)].add(min(i, j))
    up = [set() for _ in range(n)]
    for i in range(n):
        for j in low[i]:
            up[j].add(i)
    itemL = np.array([j + 1 for i in range(n) for j in sorted(low[i])], dtype=np.int32)
    itemU = np.array([j + 1 for i in range(n) for j in sorted(up[i])], dtype=np.int32)
    indexL = np.r_[0, np.cumsum([len(s) for s in low])].astype(np.int32)
    indexU = np.r_[0, np.cumsum([len(s) for s in up])].astype(np.int32)
    blk = {(i, j): 0.1 * rng.standard_normal((nd, nd)) for i in range(n) for j in low[i]}
    AL = np.array([blk[(i, j)] for i in range(n) for j in sorted(low[i])])
    AU = np.array([blk[(j, i)].T for i in range(n) for j in sorted(up[i])])
    D = np.array([rng.standard_normal((nd, nd)) * 0.1 + (2 + 0.1 * len(low[i]) + 0.1 * len(up[i])) * np.eye(nd) for i in range(n)])
    return BSR(n, n, indexL, itemL, indexU, itemU, D.ravel(), AL.ravel(), AU.ravel(), rng.standard_normal(nd * n), NDOF=nd)


# ------------------------------------------------------------------------------------------------------------------------
# Shapes at which the generic-block kernels leave their one-workgroup cases (tests/test_gpu_nn_shapes.py; what each one
# reaches is checked from the profile alone in tests/test_nn_shapes.py)
# ------------------------------------------------------------------------------------------------------------------------
SHAPE_NDOF = {"cube20": (1, 2, 4, 5, 6), "random": (1, 2, 4, 5, 6), "big": (1, 2)}
SSOR_NCOLOR = (8, 29)       # cube20: colours of up to 19 slices and of 1 row mod 64 (8), of 63 rows mod 64 (29)
BIG_M = {1: 81, 2: 64}      # big: 82^3 nodes at NDOF 1, 65^3 at NDOF 2 -- NDOF * N > 2048 * 256


def shape_system(name, nd):
    if name == "cube20":
        return cube_system(nd, 20)
    if name == "random":
        return random_system(nd, 3000, 40, 7, general=True)
    if name == "big":
        return cube_system(nd, BIG_M[nd])
    raise KeyError(name)


def ilu_levels(A):
    """The level schedule of the device block ILU(0) (nn_ilu_symbolic): level(i) = 1 + the highest level in L(i), rows 1..N.
    Returns (level of every row, rows per level)."""
    N = A.N
    level = np.zeros(N, dtype=np.int64)
    iL, jL = A.indexL, A.itemL
    for i in range(N):
        cols = jL[iL[i]:iL[i + 1]] - 1
        level[i] = 1 + (level[cols].max() if cols.size else 0)
    return level, np.bincount(level)[1:]


def ssor_layout(A, perm, colorindex, lower):
    """Slice widths of the device SSOR sweep layout (nn_ssor_setup): per colour its rows in ascending old id, padded to whole
    slices of 64; a row's entries are its internal neighbours numbered before (lower) / after it in the colour ordering.
    perm: new -> old (1-based, oracle.Precond.perm).  Returns (slices per colour, width of every slice)."""
    N = A.N
    iperm = np.empty(N, dtype=np.int64)
    iperm[perm - 1] = np.arange(N)
    nbr = [[] for _ in range(N)]
    for idx, item in ((A.indexL, A.itemL), (A.indexU, A.itemU)):
        rows = np.repeat(np.arange(A.NP), np.diff(idx))
        keep = (rows < N) & (item - 1 < N)
        for r, c in zip(rows[keep], item[keep] - 1):
            nbr[r].append(c)
    cnt = np.array([sum((iperm[c] < iperm[i]) == lower for c in nbr[i]) for i in range(N)])
    slices, widths = [], []
    for k in range(len(colorindex) - 1):
        rows = np.sort(perm[colorindex[k]:colorindex[k + 1]] - 1)
        c = np.zeros(-(-rows.size // 64) * 64, dtype=np.int64)
        c[:rows.size] = cnt[rows]
        slices.append(c.size // 64)
        widths += list(c.reshape(-1, 64).max(axis=1))
    return np.array(slices), np.array(widths)


def spmv_widths(A):
    """Slice widths of the device SpMV layout: rows 1..N in order, 64 per slice, each row D + its L and U blocks."""
    n = 1 + np.diff(A.indexL)[:A.N] + np.diff(A.indexU)[:A.N]
    c = np.zeros(-(-A.N // 64) * 64, dtype=np.int64)
    c[:A.N] = n
    return c.reshape(-1, 64).max(axis=1)


def dense(A):
    """Dense (NDOF*N)^2 image of the internal rows / columns (tests only)."""
    nd, N = A.NDOF, A.N
    M = np.zeros((nd * N, nd * N))
    D = A.D.reshape(-1, nd, nd)
    AL = A.AL.reshape(-1, nd, nd)
    AU = A.AU.reshape(-1, nd, nd)
    for i in range(N):
        M[nd * i:nd * i + nd, nd * i:nd * i + nd] = D[i]
        for j in range(A.indexL[i], A.indexL[i + 1]):
            k = A.itemL[j] - 1
            M[nd * i:nd * i + nd, nd * k:nd * k + nd] = AL[j]
        for j in range(A.indexU[i], A.indexU[i + 1]):
            k = A.itemU[j] - 1
            if k < N:
                M[nd * i:nd * i + nd, nd * k:nd * k + nd] = AU[j]
    return M
