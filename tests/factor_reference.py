"""Reference, tested quantity and a-priori bound for the subdomain factorisation (dot_amd/csrc/k_tilefactor.hip, scheduled by
tile_factor.hpp), host only.  tests/test_factor_reference.py checks all of it on the CPU, tests/test_gpu_factor_accuracy.py holds the
device's factors to it.

INPUTS.  Per subdomain the two arrays the handle returns in ascending vertex order: H_s (partMatrix(p, inverse=False), the doubles the
device assembled) and X_s (inverse=True).  `Layout` permutes both into the nested-dissection order the tiles live in (the rows
dot_amd.sharding.plan_layout gives, `pos`); only the live rows are kept, each with the 64 x 64 tile its row lies in -- the identity
padding is decoupled from them exactly (H has no entry between a padding row and a live one) and the ABI returns none of it.

REFERENCE.  `upper_factor_and_inverse`: R with H = R^T R (upper) and Q = R^-1 in numpy.longdouble by a plain left-looking blocked
algorithm on panels of 40 rows -- no tile, no task list.  Cross-checked against mpmath at 60 digits up to 64 x 64.

TESTED QUANTITY.  The device stores X = Q^T (lower triangular in dissection order); one application computes z = X^T X r, which is
H^-1 r exactly when  F = X H X^T - I  vanishes.  F is invariant under the permutation.  Evaluated as it stands, even in longdouble,
F is blind below 2^-64 n |X| |H| |X|^T (X H is a triangle by cancellation), which is far above the bound's small components.
`Reference.residual` evaluates it from the doubles read back without that cancellation: with d = X^T - Q_ref (formed in
longdouble: exact for neighbouring numbers, then rounded), E_ref = R_ref Q_ref - I and dH_ref = H - R_ref^T R_ref (longdouble,
once per matrix),  W = R_ref d + E_ref  and  F = W + W^T + W^T W + X dH_ref X^T.  The products of the small d run in double;
their rounding error (at most 2 (n + 4) u |R| |d|, second order in u) is ADDED to |F| before it is compared.

BOUND.  The algorithm as tile_factor.hpp states it, on tiles j, k, m of 64 rows (u = 2^-53, hats = computed):
    DIAG(j)   G = H_jj - sum_m R_mj^T R_mj ;  Q_jj = chol(G)^-1
    ROW(k,j)  G = H_kj - sum_m R_mk^T R_mj ;  R_kj = Q_kk^T G
    INV(i,j)  Q_ij = -(sum_m Q_im R_mj) Q_jj
and inside a diagonal tile the same three steps on halves, 64 -> 32 -> 16 -> 8 -> 4, the 4 x 4 blocks by scalar code.
With R^_jj := Q^_jj^-1 write R^^T R^ = H + dH and Q^ R^ = I + E'.  Then R^ Q^ = I + E with E = R^ E' R^^-1 and
    F = Q^^T H Q^ - I = E + E^T - Q^^T dH Q^ + (second order),
so |F| <= |R| |E'| |Q| + (|R| |E'| |Q|)^T + |Q|^T |dH| |Q|.  The factors |R| ... |Q| around E' are the price of F involving R Q
where the inversion makes only Q R = I small; nothing here is condition-free.
  * Sums.  A tile entry's sum has at most 64 Lmax + 1 terms (Lmax = the most products any one tile receives, all its eager tasks
    together, taken from the task list); whatever the order -- the list's, the eager grouping (DOTMI_TILE_EAGER_MIN, .._RMUL), the half
    tiles of tile_gemm_kernel, the order inside v_mfma_f64_16x16x4_f64 -- the computed sum is off by at most (terms + 1) u sum |terms|
    when every product and every addition commits at most one rounding (Higham, Accuracy and Stability, section 4.2: any order).
    Partial sums stored and read back are exact.  So the error of G is at most c_acc u S_kj,  c_acc = 64 Lmax + 2,
    S = |H| + |R|^T |R|.
  * Post-multiplications.  R^_kj = Q^_kk^T G^ + d, |d| <= c_post u |Q_kk|^T |G|, c_post = 65 (64 terms);  R^_kk^T d is what
    reaches dH_kj, and |G| <= |R_kk|^T |R_kj| to first order: the term (|Q_kk| |R_kk|)^T (|R|^T |R|)_kj.  TP_RMUL likewise leaves
    |E'_ij| <= (c_acc + c_post) u (|Q| |R|)_ij (I + |Q_jj| |R_jj|).  With D = I + blockdiag_64(|Q| |R|) both are  D^T S  and
    (|Q| |R|) D.  Replacing R_jj by Q^_jj^-1 moves the diagonal tile's own inverse residual into dH_jj:
    |E'_jj|^T |G| + |G| |E'_jj|, of the same form -- the constant of dH is doubled for it.
  * Inside a diagonal tile the steps repeat on four levels of halves; the blocks |Q_kk| |R_kk| of every level are sub-blocks of
    products of non-negative terms that blockdiag_64(|Q| |R|) contains, so D covers them.  Per level one Schur update (32 terms
    and the subtraction: 34) and one product per side (33):  c_rec = 4 (34 + 33) = 268.
  * The 4 x 4 blocks: at most 4 terms, one scaling, and the pivot's root and reciprocal root from sqrt_rsqrt -- two products,
    six multiply-adds in two Goldschmidt steps, two in the residual correction, the doubling exact: 10 operations at an ASSUMED
    one rounding of u each, first order (the hardware estimate's own error is removed quadratically by the two steps:
    2^-26 -> 2^-52 -> below u; the correction leaves the root to the same 10 u).  c_leaf = 4 + 1 + 10 = 15.  The one-row-per-lane
    base (DOTMI_FAST_DIAG=0) takes IEEE sqrt and division and 16 terms: less than c_rec's two lowest levels plus c_leaf.
    c = c_acc + c_post + c_rec + c_leaf = 64 Lmax + 350.
                |dH| <= 2 c u (D^T S + S D),      |E'| <= c u (|Q| |R|) D,
                B = (1 + 1e-6) [ |Q|^T |dH| |Q| + |R| |E'| |Q| + (|R| |E'| |Q|)^T ]
evaluated from |R_ref|, |Q_ref|, |H|; the factor 1 + 1e-6 covers the second-order terms (each at most max B <= 1e-7 times a first-
order one: tests/test_factor_reference.py asserts max B <= 1e-7 for every case) and the double evaluation of B itself.
No constant comes from a run of the kernels, and none had to be taken from the float64 restatement.

Out of scope: the two-level form (DOTMI_TWO_LEVEL=1) has no explicit X_s."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TILE = 64
C_POST, C_REC, C_LEAF = 65, 4 * (34 + 33), 15
TF_FACT, TF_INV = 0, 1
TP_STORE, TP_DIAG, TP_ROW, TP_NEG, TP_RMUL = 0, 1, 2, 3, 4
POST_NAME = {TP_STORE: "STORE", TP_DIAG: "DIAG", TP_ROW: "ROW", TP_NEG: "NEG", TP_RMUL: "RMUL"}


def constant(lmax):
    """c of the bound for a schedule whose busiest tile receives lmax products"""
    return 64 * lmax + 2 + C_POST + C_REC + C_LEAF


# ---- layout: ascending vertex order <-> dissection order, tile patterns ------------------------------------------------------------
class Layout:
    """One subdomain of a planned layout: rows[k] = the memory row of scalar k of the ascending-vertex order, order = the scalars
    sorted by row (dissection order), tile[i] = tile of the i-th live row, and the tile patterns the planner derives."""

    def __init__(self, T, verts, pos, nmax):
        self.nmax, self.nt = int(nmax), int(nmax) // TILE
        self.rows = (np.asarray(pos, dtype=np.int64)[:, None] + np.arange(3)[None, :]).ravel()
        self.order = np.argsort(self.rows, kind="stable")
        self.live_rows = self.rows[self.order]
        self.tile = self.live_rows // TILE
        self.n = self.rows.size
        self.live = np.zeros(self.nt, dtype=np.uint8)
        self.live[self.tile] = 1
        # upper tile pattern of H_s, the rule of plan_factor_schedule (block_plan.hpp): the corners of every 3 x 3 block between two
        # vertices of the part that share a tet (of any part: H_s is a submatrix of H)
        loc = np.full(int(np.max(T)) + 1, -1, dtype=np.int64)
        loc[np.asarray(verts)] = np.arange(len(verts))
        lt = loc[np.asarray(T)]
        pat = np.zeros((self.nt, self.nt), dtype=np.uint8)
        p = np.asarray(pos, dtype=np.int64)
        for a in range(4):
            for b in range(4):
                ok = (lt[:, a] >= 0) & (lt[:, b] >= 0)
                ra, rb = p[lt[ok, a]], p[lt[ok, b]]
                for da in (0, 2):
                    for db in (0, 2):
                        I, J = (rb + db) // TILE, (ra + da) // TILE
                        pat[I[I <= J], J[I <= J]] = 1
        self.hpat = pat
        self.rpat, self.qpat = symbolic(self.nt, self.live, pat)
        # padding rows that can reach a live entry of the factor: inside a live tile, with a live row behind them in the tile or a
        # later tile that the symbolic factor couples to theirs (a padding row at the very end of its sub-tree touches nothing)
        pad = np.setdiff1d(np.arange(self.nmax), self.live_rows)
        last = {t: self.live_rows[self.tile == t].max() for t in np.unique(self.tile)}
        self.pad_rows = np.array([r for r in pad if r // TILE in last and (r < last[r // TILE] or self.rpat[r // TILE, r // TILE + 1:].any())],
                                 dtype=np.int64)

    def to_dissection(self, M):
        return np.asarray(M)[np.ix_(self.order, self.order)]

    def padded(self, Hd):
        """the nmax x nmax matrix the tiles hold: Hd on the live rows, the identity on the padding"""
        P = np.eye(self.nmax)
        P[np.ix_(self.live_rows, self.live_rows)] = Hd
        return P

    def live_sizes(self):
        """live rows per tile"""
        return np.bincount(self.tile, minlength=self.nt)

    def mixed_blocks(self, q):
        """aligned q x q diagonal blocks that hold live rows AND identity padding"""
        lv = np.zeros(self.nmax, dtype=bool)
        lv[self.live_rows] = True
        k = lv.reshape(-1, q).sum(axis=1)
        return int(((k > 0) & (k < q)).sum())


def symbolic(nt, live, hpat):
    """struct(R) and struct(Q) on tiles as plan_subdomain_tiles derives them (symbolic factorisation, symbolic inversion)"""
    P = np.array(hpat, dtype=bool)
    for j in range(nt):
        if live[j]:
            P[j, j] = True
    for k in range(nt):
        if not live[k]:
            continue
        row = [j for j in range(k + 1, nt) if P[k, j]]
        for a in range(len(row)):
            for b in range(a, len(row)):
                P[row[a], row[b]] = True
    qcol = [[] for _ in range(nt)]
    Qp = np.zeros((nt, nt), dtype=bool)
    for j in range(nt):
        if not live[j]:
            continue
        inn = np.zeros(nt, dtype=bool)
        inn[j] = True
        for m in range(j):
            if P[m, j]:
                inn[qcol[m]] = True
        qcol[j] = [i for i in range(j + 1) if inn[i]]
        Qp[qcol[j], j] = True
    return P, Qp


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def upper_factor_and_inverse(H, nb=40):
    """(R, Q) in longdouble: H = R^T R, R upper, Q = R^-1.  Left-looking on panels of nb rows; raises on a non-positive pivot."""
    H = np.asarray(H, dtype=LD)
    n = H.shape[0]
    R = np.zeros((n, n), dtype=LD)
    for j0 in range(0, n, nb):
        j1 = min(n, j0 + nb)
        A = H[j0:j1, j0:] - R[:j0, j0:j1].T @ R[:j0, j0:]
        for k in range(j1 - j0):
            if not A[k, k] > 0:
                raise np.linalg.LinAlgError(f"pivot {j0 + k} is not positive")
            A[k, k:] /= np.sqrt(A[k, k])
            for i in range(k + 1, j1 - j0):
                A[i, i:] -= A[k, i] * A[k, i:]
            A[k + 1:, k] = 0
        R[j0:j1, j0:] = A
    Q = np.zeros((n, n), dtype=LD)
    for j1 in range(n, 0, -nb):
        j0 = max(0, j1 - nb)
        D = np.zeros((j1 - j0, j1 - j0), dtype=LD)          # the panel's own inverse, row by row from the bottom
        for i in range(j1 - j0 - 1, -1, -1):
            D[i, i] = 1 / R[j0 + i, j0 + i]
            D[i, i + 1:] = -(R[j0 + i, j0 + i + 1:j1] @ D[i + 1:, i + 1:]) * D[i, i]
        Q[j0:j1, j0:j1] = D
        if j1 < n:
            Q[j0:j1, j1:] = -D @ (R[j0:j1, j1:] @ Q[j1:, j1:])
    return R, Q


def bound(H, R, Q, tile, lmax):
    """B (double, n x n) from |H|, |R_ref|, |Q_ref| in dissection order; tile[i] = tile of row i; lmax = most products of one tile"""
    aH, aR, aQ = (np.abs(np.asarray(x)).astype(np.float64) for x in (H, R, Q))
    c = constant(lmax) * U
    S = aH + aR.T @ aR
    QR = aQ @ aR
    same = np.asarray(tile)[:, None] == np.asarray(tile)[None, :]
    D = np.eye(len(aH)) + np.where(same, QR, 0.0)
    dH = 2 * c * (D.T @ S + S @ D)
    E = aR @ (c * (QR @ D)) @ aQ
    return (1 + 1e-6) * (aQ.T @ dH @ aQ + E + E.T)


class Reference:
    """what the tests need of one matrix H (dissection order, live rows): R_ref, Q_ref, B, and the pieces of `residual`"""

    def __init__(self, Hd, tile, lmax):
        # (the factorisation reads one triangle: H is that triangle mirrored -- the device's own read-back is symmetric bit for bit,
        # the oracle's sums may differ between the triangles in their last bits)
        Hd = np.asarray(Hd, dtype=np.float64)
        self.H = np.triu(Hd) + np.triu(Hd, 1).T
        self.tile = np.asarray(tile)
        Hl = self.H.astype(LD)
        self.R, self.Q = upper_factor_and_inverse(Hl)
        self.B = bound(Hl, self.R, self.Q, tile, lmax)
        n = len(Hl)
        # the reference's own residuals, longdouble: of the order 2^-64 n |R| |Q| and 2^-64 n |R|^T |R|
        self.E = (self.R @ self.Q - np.eye(n, dtype=LD)).astype(np.float64)
        dH = (Hl - self.R.T @ self.R).astype(np.float64)
        self.R64, self.Q64 = self.R.astype(np.float64), self.Q.astype(np.float64)
        self.F0 = self.Q64.T @ dH @ self.Q64
        self.aR = np.abs(self.R64)

    def residual(self, X):
        """|F(X)| plus the evaluation's own rounding error, as doubles (inf everywhere if X is not finite)"""
        X = np.asarray(X, dtype=np.float64)
        if not np.isfinite(X).all():
            return np.full(X.shape, np.inf)
        d = (X.T.astype(LD) - self.Q).astype(np.float64)
        W = self.R64 @ d + self.E
        F = W + W.T + W.T @ W + self.F0
        ev = self.aR @ np.abs(d)
        ev = 2 * (len(X) + 4) * U * (ev + ev.T) + 1e-6 * np.abs(F)
        return np.abs(F) + ev

    def residual_direct(self, X):
        """|X H X^T - I| evaluated in longdouble as it stands (slow, and blind below 2^-64 n |X| |H| |X|^T: X H is a lower
        triangle by cancellation); tests/test_factor_reference.py compares `residual` with it"""
        XL = np.asarray(X, dtype=np.float64).astype(LD)
        Hl = self.H.astype(LD)
        F = np.abs(XL @ (Hl @ XL.T) - np.eye(len(XL), dtype=LD)).astype(np.float64)
        aX = np.abs(np.asarray(X, dtype=np.float64))
        return F, 2.0 ** -63 * (len(XL) + 2) * (aX @ np.abs(self.H) @ aX.T + np.eye(len(XL)))


def worst(res, B):
    """(ratio, i, j) of the component with the largest res / B (anything above a zero bound, or not finite, counts as infinite)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(B > 0, res / np.where(B > 0, B, 1.0), np.where(res > 0, np.inf, 0.0))
    r = np.where(np.isfinite(res), r, np.inf)
    k = int(np.argmax(r))
    return float(r.ravel()[k]), k // r.shape[1], k % r.shape[1]


def shape_violations(Xd, lay):
    """entries of X (dissection order) that must be exact zeros and are not: above the diagonal (X = Q^T is lower triangular) and
    in tiles outside the symbolic pattern of Q, which no task writes"""
    ti, tj = lay.tile[:, None], lay.tile[None, :]
    must = np.triu(np.ones_like(Xd, dtype=bool), 1) | ~lay.qpat[tj, ti]
    return np.argwhere(must & (Xd != 0.0))


# ---- the schedule restated in float64 (tests/test_factor_reference.py) ------------------------------------------------------------
def chol_inv_halves(G, pivot_hook=None, base=0):
    """X = chol(G)^-1 (lower) by the 2 x 2 recursion of block_chol_inv down to 4 x 4 blocks in scalar code, in float64.
    pivot_hook(index) -> relative error of that pivot's root (the reciprocal root consistent with it), or None"""
    n = len(G)
    if n == 4:
        A = np.array(G, dtype=np.float64)
        L = np.zeros((4, 4))
        for k in range(4):
            root = np.sqrt(A[k, k])
            if pivot_hook is not None:
                root = root * (1.0 + pivot_hook(base + k))
            rr = 1.0 / root
            L[k, k] = root
            L[k + 1:, k] = A[k + 1:, k] * rr
            for j in range(k + 1, 4):
                A[j:, j] -= L[j:, k] * L[j, k]
        X = np.zeros((4, 4))
        for c in range(4):
            x = np.zeros(4)
            x[c] = 1.0
            for k in range(4):
                x[k] = x[k] / L[k, k]
                x[k + 1:] -= L[k + 1:, k] * x[k]
            X[:, c] = x
        return np.tril(X)
    h = n // 2
    X11 = chol_inv_halves(G[:h, :h], pivot_hook, base)
    R12 = X11 @ G[:h, h:]
    X22 = chol_inv_halves(G[h:, h:] - R12.T @ R12, pivot_hook, base + h)
    X = np.zeros((n, n))
    X[:h, :h], X[h:, h:] = X11, X22
    X[h:, :h] = -X22 @ (R12.T @ X11)
    return X


def tile_origin(off, roff, rld, c0):
    """(i, j) of the tile whose origin is `off` in a buffer with the row-block table (roff, rld, c0)"""
    for j in range(len(roff)):
        if rld[j] > 0 and roff[j] <= off < roff[j] + rld[j]:
            return int(off - roff[j]) // TILE + int(c0[j]), j
    raise AssertionError(off)


def run_tasks(plan_out, lay, Hpad, order="schedule", mutation=None, magnitudes=None):
    """The task list of dotmi_plan_tile_schedule (plan_out = what tests/test_tile_schedule.plan returns, planned with c0 = 0) executed
    in float64 on the padded matrix Hpad by the executor of tests/test_tile_schedule.py (execute_levels: level after level, with
    its assertions on the levels), with its hooks set here.  order: "schedule" (every product list as it stands), "reversed",
    "pairwise" (the products of a task summed as a balanced tree, then added); the diagonal tiles by the kernels' 2 x 2 recursion
    (chol_inv_halves).  mutation: None or ("drop", task, k) / ("sign", task) / ("pivot", row, eps) / ("pad", row), see
    tests/test_factor_reference.py.
    magnitudes: a dict that receives {(task, k): max |product k of the task|, (task, "out"): max |the tile it writes|}.
    Returns X (n x n, dissection order, live rows) = Q^T as the factor buffer holds it."""
    from tests import test_tile_schedule as TS
    tasks, prods, nlev, storage, roff, rld = plan_out
    nt = lay.nt
    c0 = np.zeros(nt, dtype=np.int32)
    mut = mutation or (None,)

    class H(TS.Hooks):
        def products(self, t, plist):
            if mut[0] == "drop" and mut[1] == t:
                plist = plist[:mut[2]] + plist[mut[2] + 1:]
            return plist[::-1] if order == "reversed" else plist

        def add(self, acc, terms):
            if order != "pairwise":
                return TS.Hooks.add(self, acc, terms)
            terms = list(terms)
            while len(terms) > 1:
                terms = [terms[k] + terms[k + 1] if k + 1 < len(terms) else terms[k] for k in range(0, len(terms), 2)]
            return acc + terms[0] if terms else acc

        def diag(self, t, acc):
            j = tile_origin(int(tasks[t, 10]), roff, rld, c0)[1]
            hook = None
            if mut[0] == "pivot" and mut[1] // 64 == j:
                hook = lambda r: mut[2] if r == mut[1] % 64 else 0.0
            return chol_inv_halves(acc, hook).T

        def rmul_sign(self, t):
            return 1.0 if (mut[0] == "sign" and mut[1] == t) else -1.0

        def done(self, t, terms, out):
            if magnitudes is not None:
                for k, P in enumerate(terms):
                    magnitudes[t, k] = float(np.abs(P).max())
                magnitudes[t, "out"] = float(np.abs(out).max())

    Hp = Hpad
    if mut[0] == "pad":
        Hp = Hpad.copy()
        Hp[mut[1], mut[1]] = 0.0
    with np.errstate(all="ignore"):
        tile = TS.execute_levels(plan_out, nt, lay.live, lay.hpat, c0, Hp, H())
    Qp = np.zeros((lay.nmax, lay.nmax))
    for j in range(nt):
        if lay.live[j]:
            for i in range(j + 1):
                if lay.qpat[i, j]:
                    blk = tile(roff[j] + 64 * i, rld[j])
                    Qp[64 * i:64 * i + 64, 64 * j:64 * j + 64] = np.triu(blk) if i == j else blk
    return Qp[np.ix_(lay.live_rows, lay.live_rows)].T


def most_products(plan_out):
    """Lmax: the most products any one tile receives, its eager tasks and its last task together (tasks of one tile share their c tile)"""
    tasks = plan_out[0]
    tot = {}
    for t in tasks:
        tot[int(t[6])] = tot.get(int(t[6]), 0) + int(t[4])
    return max(tot.values()) if tot else 0


def tile_writers(plan_out, nt):
    """{(i, j): [post names]} of the tasks that write tile (i, j), factor buffer ("Q") and work buffer ("R") apart"""
    tasks, prods, nlev, storage, roff, rld = plan_out
    out = {}
    z = np.zeros(nt)
    for t in np.argsort(tasks[:, 0], kind="stable"):
        post, nprod, ooff = int(tasks[t, 3]), int(tasks[t, 4]), int(tasks[t, 10])
        buf = "Q" if ooff < storage else "R"
        ij = tile_origin(ooff - storage if ooff >= storage else ooff, roff, rld, z)
        out.setdefault((buf,) + ij, []).append(f"{POST_NAME[post]}({nprod})")
    return out
