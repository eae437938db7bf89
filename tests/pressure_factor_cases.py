"""Synthetic cases for `mdq_ipcs_factorize_pressure` and a plain numpy restatement of its documented rule.

The kernel reads a scaled SPD matrix in SELL-64 and the vertex coordinates, nothing else of a mesh: the cases here are
weighted graph Laplacians K = D^-1/2 (L + sigma I) D^-1/2 (unit diagonal, like `K1s`) on point sets whose bisection
lands exactly on, or one beyond, every size the kernel branches on.  All coordinates are integers or multiples of
2^-4, so the 51-bit truncation of the kernel's sort key loses nothing and the rule below is exact.

The rule (mdq_pressure_factor.hip):
  bisection  three levels; per part the axis of larger extent (x on a tie); sort by (truncated coordinate key, vertex
             id); the upper sz - sz // 2 go to part 2 g + 1, the rest (and a part of size 1) to 2 g;
  separator  v is a separator if some c != v with K[v, c] != 0 lies in a lower part;
  ordering   the interiors of every part that has any, ascending vertex id inside a part, then the separator ascending;
  factors    W_s = inv(K[I_s, I_s]), F_s = W_s K[I_s, G_s] (G_s: separator vertices touching I_s, ascending),
             Sinv = inv(K[G, G] - sum_s K[G_s, I_s] F_s), the inverses symmetrised.
Nothing here imports meshdqn_amd.pressure_direct: `factor_reference` is a second statement of the layout, not a copy."""
from collections import namedtuple

import numpy as np

NVMAX, MMAX, NGMAX, GMAX, PARTS = 1024, 112, 112, 48, 8
# capacities of the device tables (== IpcsBatch.PD_DEVICE_CAP, asserted by the GPU test)
CAP = dict(NPART=8, NPW=8 * 112 * 112, NPF=8 * 112 * 48, NPGI=8 * 48, NPS=112 * 112 + 8 * 48 * 48, NPGK=4096)
SIGMA = 0.01        # cond(L + sigma I) <= (lambda_max + sigma) / sigma: lambda_max <= 2 * 6 * 2 on the grids -> <= 2401


# ------------------------------------------------------------------------------------------------ generators
def _scaled_laplacian(nv, edges, seed):
    rng = np.random.default_rng(seed)
    e = np.unique(np.sort(np.asarray(edges, np.int64).reshape(-1, 2), axis=1), axis=0)
    assert (e[:, 0] != e[:, 1]).all()
    w = rng.uniform(0.5, 2.0, e.shape[0])
    A = np.zeros((nv, nv))
    A[e[:, 0], e[:, 1]] = -w
    A[e[:, 1], e[:, 0]] = -w
    A[np.arange(nv), np.arange(nv)] = SIGMA - A.sum(axis=1)
    sd = np.sqrt(np.diag(A))
    K = A / np.outer(sd, sd)
    np.fill_diagonal(K, 1.0)
    assert np.array_equal(K, K.T)
    return K


def grid(nx, ny, seed=1):
    """nx x ny vertices at the integer points (i, j), id = j nx + i; couplings right, up and diagonal (i + 1, j + 1)."""
    jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    coords = np.stack([ii.ravel(), jj.ravel()], 1).astype(np.float64)
    vid = jj * nx + ii
    edges = [np.stack([vid[:, :-1].ravel(), vid[:, 1:].ravel()], 1), np.stack([vid[:-1].ravel(), vid[1:].ravel()], 1),
             np.stack([vid[:-1, :-1].ravel(), vid[1:, 1:].ravel()], 1)]
    return coords, _scaled_laplacian(nx * ny, np.concatenate(edges), seed)


def line_clusters(k, g, shift=0.0, same_x=False, seed=2):
    """8 k vertices at x = i + shift (all at x = shift with `same_x`), y = 0: a path inside each block of k, one link between
    consecutive blocks, and g extra couplings (j % k, k + j) from block 1 into block 0."""
    nv = 8 * k
    assert g < k
    coords = np.zeros((nv, 2))
    coords[:, 0] = shift if same_x else np.arange(nv) + shift
    edges = [(i, i + 1) for i in range(nv - 1)] + [(j % k, k + j) for j in range(g)]
    return coords, _scaled_laplacian(nv, edges, seed)


# name, generator, expected status, and what the size table of the case claims (None: no claim):
# nv, interiors (list: the exact sizes; int: the largest), nG, largest gs, number of parts
Case = namedtuple("Case", "name make status nv m nG gs nparts")
CASES = [
    Case("grid(1,1)", lambda: grid(1, 1), 0, 1, [1], 0, 0, 1),
    Case("grid(2,1)", lambda: grid(2, 1), 0, 2, [1], 1, 1, 1),
    Case("grid(3,1)", lambda: grid(3, 1), 0, 3, [1], 2, 1, 1),
    Case("grid(7,1)", lambda: grid(7, 1), 0, 7, [1], 6, 1, 1),
    Case("grid(5,4)", lambda: grid(5, 4), 0, 20, [2, 1, 1], 16, 4, 3),
    Case("grid(9,9)", lambda: grid(9, 9), 0, 81, None, 39, None, 8),
    Case("grid(13,11)", lambda: grid(13, 11), 0, 143, None, 48, 15, 8),
    Case("grid(40,22)", lambda: grid(40, 22), 0, 880, 110, 103, 32, 8),
    Case("grid(56,16)", lambda: grid(56, 16), 0, 896, 112, 101, 30, 8),
    Case("grid(112,8)", lambda: grid(112, 8), 0, 896, 112, 56, 16, 8),
    Case("grid(903,1)", lambda: grid(903, 1), 0, 903, [112] * 8, 7, 2, 8),
    Case("grid(904,1)", lambda: grid(904, 1), -2, 904, 113, 7, None, 8),
    Case("grid(28,32)", lambda: grid(28, 32), -2, 896, 112, 113, None, 8),
    Case("grid(1024,1)", lambda: grid(1024, 1), -2, 1024, 128, None, None, 8),
    Case("line_clusters(112,48)", lambda: line_clusters(112, 48), 0, 896, 112, 54, 48, 8),
    Case("line_clusters(60,49)", lambda: line_clusters(60, 49), -4, 480, 60, 55, 49, 8),
    Case("line_clusters(20,5,shift=-75.5)", lambda: line_clusters(20, 5, shift=-75.5), 0, 160, None, 11, None, 8),
    Case("line_clusters(20,5,same_x)", lambda: line_clusters(20, 5, same_x=True), 0, 160, None, 11, None, 8),
]
CASE = {c.name: c for c in CASES}
_made = {}


def make(name):
    """(coords, K) of a case, built once per process; callers must not modify them."""
    if name not in _made:
        coords, K = CASE[name].make()
        coords.setflags(write=False)
        K.setflags(write=False)
        _made[name] = (coords, K)
    return _made[name]


def stored_zero_pattern(K):
    """The explicit-zero variant: the pairs two couplings apart that are not coupled themselves are STORED, with value 0.
    Many of them cross parts, so a kernel that took a stored zero for a coupling would grow the separator."""
    A = (K != 0).astype(np.int64)
    return ((A @ A) != 0) & (K == 0)


# ------------------------------------------------------------------------------------------------ packing
def pack(K, zeros=None):
    """SELL-64 arrays (sl_off, sl_col, values) of K: CSR with ascending columns and the diagonal included (plus the pattern
    `zeros` stored with value 0), padding = the row's own index with value 0."""
    from meshdqn_amd.topology import MeshTopology
    pat = (K != 0) | np.eye(K.shape[0], dtype=bool)
    if zeros is not None:
        assert not (zeros & pat).any()
        pat = pat | zeros
    rows, cols = np.nonzero(pat)                                    # row-major: columns ascend inside a row
    rowptr = np.zeros(K.shape[0] + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=K.shape[0]), out=rowptr[1:])
    sl_off, sl_col, pos = MeshTopology.sell_layout(rowptr, cols.astype(np.int32))
    vals = np.zeros(sl_col.size)
    vals[pos] = K[rows, cols]
    return sl_off, sl_col, vals


def unpack(sl_off, sl_col, vals, nv):
    """(dense matrix, stored pattern) of SELL-64 arrays, by the kernel's walk of a row: ascending columns are entries,
    what follows them must be padding - the row's own index with value 0."""
    D, stored = np.zeros((nv, nv)), np.zeros((nv, nv), bool)
    for r in range(nv):
        o, w = int(sl_off[r >> 6]), (int(sl_off[(r >> 6) + 1]) - int(sl_off[r >> 6])) >> 6
        prev = -1
        for j in range(w):
            p = o + j * 64 + (r & 63)
            if sl_col[p] > prev:
                prev = sl_col[p]
                D[r, prev], stored[r, prev] = vals[p], True
            else:
                assert sl_col[p] == r and vals[p] == 0.0, (r, j)
    return D, stored


def batch_arrays(items, NV=None):
    """Host arrays of one launch.  `items`: per environment (coords, K) or (coords, K, zeros), or an int = a bare `nv`
    outside [1, 1024] with no matrix behind it.  Ragged nv; NV = the largest, rounded up to 64."""
    nvs = [it if isinstance(it, int) else it[1].shape[0] for it in items]
    if NV is None:
        NV = max(64, -(-max(nvs) // 64) * 64)
    packed = [None if isinstance(it, int) else pack(it[1], it[2] if len(it) > 2 else None) for it in items]
    NSE1 = max([64] + [p[1].size for p in packed if p is not None])
    B = len(items)
    h = dict(nv=np.array(nvs, np.int32), coords=np.zeros((B, NV, 2)), sl1_off=np.zeros((B, NV // 64 + 2), np.int32),
             sl1_col=np.zeros((B, NSE1), np.int32), K1s=np.zeros((B, NSE1)))
    for b, (it, p) in enumerate(zip(items, packed)):
        if p is None:
            continue
        n = nvs[b]
        h["coords"][b, :n] = it[0]
        h["sl1_off"][b, :p[0].size] = p[0]
        h["sl1_col"][b, :p[1].size] = p[1]
        h["K1s"][b, :p[2].size] = p[2]
    return h, NV, NSE1


# ------------------------------------------------------------------------------------------------ the rule
def _ordered_key51(x):
    """Order-preserving map double -> uint64 (sign bit flipped for x >= 0, all bits for x < 0), top 51 bits."""
    u = np.ascontiguousarray(x, np.float64).view(np.uint64)
    neg = (u >> np.uint64(63)).astype(bool)
    return np.where(neg, ~u, u | np.uint64(1 << 63)) >> np.uint64(13)


def partition_reference(coords, K):
    """(part (nv,), separator flags (nv,), ordering (nv,)) of the documented rule."""
    nv = K.shape[0]
    coords = np.asarray(coords, np.float64)[:nv]
    part = np.zeros(nv, np.int64)
    for _ in range(3):
        new = part.copy()
        for g in np.unique(part):
            idx = np.flatnonzero(part == g)
            ext = coords[idx].max(axis=0) - coords[idx].min(axis=0)
            ax = 0 if ext[0] >= ext[1] else 1
            order = idx[np.lexsort((idx, _ordered_key51(coords[idx, ax])))]
            new[order] = 2 * g
            if idx.size > 1:
                new[order[idx.size // 2:]] = 2 * g + 1
        part = new
    A = K != 0
    A[np.arange(nv), np.arange(nv)] = False
    lower = part[None, :] < part[:, None]                           # [v, c]: c lies in a lower part than v
    sep = (A & lower).any(axis=1)
    node = np.concatenate([np.flatnonzero((part == s) & ~sep) for s in range(PARTS)] + [np.flatnonzero(sep)])
    return part, sep, node.astype(np.int32)


def sizes_reference(coords, K):
    """What the limits are measured on: interiors per subdomain, nG, gs per subdomain, number of K[G, I] entries."""
    part, sep, node = partition_reference(coords, K)
    G = np.flatnonzero(sep)
    interiors = [np.flatnonzero((part == s) & ~sep) for s in range(PARTS)]
    interiors = [I for I in interiors if I.size]
    gs = [int((K[np.ix_(I, G)] != 0).any(axis=0).sum()) for I in interiors]
    kgi = int((K[np.ix_(G, np.flatnonzero(~sep))] != 0).sum())
    return dict(nv=K.shape[0], m=[int(I.size) for I in interiors], nG=int(G.size), gs=gs, kgi=kgi, nparts=len(interiors))


def refusal_reference(sz, cap=CAP):
    """(status code, subdomain at which a -4 stops or None) the header documents for these sizes at these capacities,
    in the order the kernel checks."""
    if sz["nv"] < 1 or sz["nv"] > NVMAX:
        return -1, None
    if max(sz["m"]) > MMAX or sz["nG"] > NGMAX or sz["nparts"] > cap["NPART"] or \
            NGMAX * NGMAX + sz["nparts"] * GMAX * GMAX > cap["NPS"]:
        return -2, None
    if sz["kgi"] > cap["NPGK"]:
        return -3, None
    woff = foff = gioff = 0
    for s, (m, g) in enumerate(zip(sz["m"], sz["gs"])):
        if g > GMAX or woff + m * m > cap["NPW"] or foff + m * g > cap["NPF"] or gioff + g > cap["NPGI"]:
            return -4, s
        woff, foff, gioff = woff + m * m, foff + m * g, gioff + g
    return 0, None


def status_reference(sz, cap=CAP):
    return refusal_reference(sz, cap)[0]


def _sym_inv(A):
    W = np.linalg.inv(A)
    return 0.5 * (W + W.T)


def factor_reference(coords, K):
    """The tables of an accepted environment: integer ones exact, W / F / Sinv from LAPACK inverses in fp64."""
    n = K.shape[0]
    part, sep, node = partition_reference(coords, K)
    G = np.flatnonzero(sep)
    nG, nI = int(G.size), int(n - G.size)
    inv = np.empty(n, np.int64)
    inv[node] = np.arange(n)
    interiors = [np.flatnonzero((part == s) & ~sep) for s in range(PARTS)]
    interiors = [I for I in interiors if I.size]
    meta, rowblk, Ws, Fs, gis = [], np.zeros(nI, np.int32), [], [], []
    S = K[np.ix_(G, G)].copy()
    q0 = woff = foff = gioff = 0
    for s, I in enumerate(interiors):
        m = int(I.size)
        W = _sym_inv(K[np.ix_(I, I)])
        KIG = K[np.ix_(I, G)]
        loc = np.flatnonzero((KIG != 0).any(axis=0))
        F = W @ KIG[:, loc]
        S[np.ix_(loc, loc)] -= KIG[:, loc].T @ F
        meta.append((q0, m, woff, foff, loc.size, gioff))
        rowblk[q0:q0 + m] = s
        Ws.append(W.ravel(order="F"))
        Fs.append(F.ravel(order="F"))
        gis.append(loc)
        q0, woff, foff, gioff = q0 + m, woff + m * m, foff + m * loc.size, gioff + loc.size
    Sinv = _sym_inv(S) if nG else np.zeros((0, 0))
    gk_ptr, gk_col, gk_val = np.zeros(nG + 1, np.int32), [], []
    for r, v in enumerate(G):
        cols = np.flatnonzero((K[v] != 0) & ~sep)                     # ascending vertex id, as the rows are stored
        gk_col.append(inv[cols])
        gk_val.append(K[v, cols])
        gk_ptr[r + 1] = gk_ptr[r] + cols.size
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)   # noqa: E731
    return dict(n=n, nI=nI, nG=nG, nparts=len(interiors), hdr=np.array([nI, nG, len(interiors), 0], np.int32), node=node,
                meta=np.array(meta, np.int32).ravel(), rowblk=rowblk, W=cat(Ws, np.float64), F=cat(Fs, np.float64),
                gidx=cat(gis, np.int32), Sinv=Sinv.ravel(order="F"), gk_ptr=gk_ptr, gk_col=cat(gk_col, np.int32),
                gk_val=cat(gk_val, np.float64))


# ------------------------------------------------------------------------------------------------ accuracy measures
U = 2.0 ** -53


def solve_error(pd, K, seed=0):
    """Relative max error of the solve phases on these tables: x_true random, b = K x_true in long double, rounded."""
    from meshdqn_amd.pressure_direct import solve_reference
    x_true = np.random.default_rng(seed).standard_normal(K.shape[0])
    b = (K.astype(np.longdouble) @ x_true.astype(np.longdouble)).astype(np.float64)
    x = solve_reference(pd, b)
    return float(np.abs(x - x_true).max() / np.abs(x_true).max())


def exact_schur(pd, K):
    """S of the partition in `pd` (node, hdr) in long double, independent of pd's W and F: K_II^-1 K_IG by a LAPACK solve
    and one step of refinement on the long-double residual, which takes its error from cond(K_II) u down to the order of
    u - well below the cond u that an fp64 inverse, the device's or LAPACK's, carries into its own S."""
    ld = np.longdouble
    node, nI = pd["node"], pd["nI"]
    G = node[nI:]
    S = K[np.ix_(G, G)].astype(ld)
    for q0, m, _, _, _, _ in pd["meta"].reshape(-1, 6):
        I = node[q0:q0 + m]
        KII, KIG = K[np.ix_(I, I)], K[np.ix_(I, G)]
        X = np.linalg.solve(KII, KIG)
        r = (KIG.astype(ld) - KII.astype(ld) @ X.astype(ld)).astype(np.float64)
        S -= KIG.T.astype(ld) @ (X.astype(ld) + np.linalg.solve(KII, r).astype(ld))
    return S


def block_residuals(pd, K):
    """Per block (residual, floor): max|W K_II - I|, max|F - W K_IG| / max|F|, and max|Sinv S - I| against the exact S.
    The products are formed in long double, so that what is measured is the tables and not the measurement.  A floor is
    ONE rounding of the entries - u max|W| max|K_II|, u for the relative F residual, u max|Sinv| max|S| with u = 2^-53 -
    and only decides where the reference's residual is (nearly) exactly 0: blocks of one or two nodes."""
    ld = np.longdouble
    node, nI, nG = pd["node"], pd["nI"], pd["nG"]
    G = node[nI:]
    out = dict(W=[], F=[], S=None)
    for q0, m, woff, foff, g, gioff in pd["meta"].reshape(-1, 6):
        I = node[q0:q0 + m]
        W = pd["W"][woff:woff + m * m].reshape(m, m, order="F")
        KII = K[np.ix_(I, I)]
        rW = float(np.abs(W.astype(ld) @ KII.astype(ld) - np.eye(m)).max())
        out["W"].append((rW, U * float(np.abs(W).max() * np.abs(KII).max())))
        if g:
            F = pd["F"][foff:foff + m * g].reshape(m, g, order="F")
            KIG = K[np.ix_(I, G[pd["gidx"][gioff:gioff + g]])]
            rF = float(np.abs(F.astype(ld) - W.astype(ld) @ KIG.astype(ld)).max()) / float(np.abs(F).max())
            out["F"].append((rF, U))
    if nG:
        S = exact_schur(pd, K)
        Sinv = pd["Sinv"][:nG * nG].reshape(nG, nG, order="F")
        rS = float(np.abs(Sinv.astype(ld) @ S - np.eye(nG)).max())
        out["S"] = (rS, U * float(np.abs(Sinv).max() * np.abs(S).max()))
    return out
