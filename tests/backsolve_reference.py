"""The block solve on the factor AS STORED, in plain numpy, with an a-priori componentwise error bound (no GPU, no library).

What the back-solve launch (dot_amd/csrc/k_backsolve.hip) and the merge behind it must compute from the doubles of the stored
factors X_s (dotmi_part_matrix(inverse=1)) is a fixed bilinear expression:

    p_s = X_s^T (X_s r_s)                          per subdomain s, r_s = r on the subdomain's vertices
    z_v = (sum over the s that hold v of p_s[v]) / dup_v          (merge_kernel: the sum, then ONE division when dup_v > 1)

and beside it the same expression on absolute values,

    S_v = (sum over the s that hold v of (|X_s|^T (|X_s| |r_s|))[v]) / dup_v.

The bound.  u = 2^-53, gamma_m = m u / (1 - m u) (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1),
n = the largest scalar size n_s of a subdomain.  Every product and every sum of the kernels is rounded on its own (the library is
built with -ffp-contract=off; a fused multiply-add rounds once instead of twice and stays inside the same bound).  Padding columns
and structural zeros contribute exact zeros, so a sum has at most n inexact terms.
  1. t = X r.  A sum of at most n products in ANY order (lanes, butterfly, wavefronts, column chunks):
         |t^ - t| <= gamma_n |X| |r|,                 hence |t^| <= (1 + gamma_n) |X| |r|.
  2. p = X^T t^.  Again at most n products per component, in any order (rows of a pass, passes, tiles, the tile partials' sum):
         |p^ - X^T t^| <= gamma_n |X|^T |t^| <= gamma_n (1 + gamma_n) |X|^T |X| |r|
         |X^T t^ - X^T t| <= gamma_n |X|^T |X| |r|
     together  |p^_s - p_s| <= (2 gamma_n + gamma_n^2) S_s,   S_s = |X_s|^T |X_s| |r_s|.
  3. The merge: dup - 1 additions and one division, at most dup roundings (<= gamma_{dup+1}) of sum_s |p^_s| <= (1 + 2 gamma_n +
     gamma_n^2) dup S, on top of the error sum_s |p^_s - p_s| / dup <= (2 gamma_n + gamma_n^2) S it passes on:
         |z^_v - z_v| <= c(n, dup_v, u) S_v,     c(n, d, u) = (2 gamma_n + gamma_n^2) (1 + gamma_{d+1}) + gamma_{d+1}.
The reference is an evaluation of the same expression in a floating-point format of its own (unit roundoff u_ref), so it obeys the
same theorem with u_ref in place of u; and S, a sum of non-negative terms, comes out at least (1 - gamma_{2n+d+1}(u_ref)) times its
exact value.  The tolerance a device value is held to is therefore

    tol_v = (c(n, dup_v, u) + c_ref) S^_v / (1 - gamma_{2 n + dup_v + 1}(u_ref))

with c_ref = c(n, dup_v, u_ref) for reference_apply (numpy.longdouble, u_ref = 2^-64: x86 extended precision; its eps is asserted at
import) and c_ref = gamma_n (1 + gamma_{dup+1}) + gamma_{dup+1} at u_ref = u for reference_unit_columns (float64 BLAS on unit vectors:
the first pass, t = a column of X, is exact, so only step 2 once and step 3 remain).  No constant in it was measured anywhere.
Where S_v = 0 every term of z_v is an exact zero and tol_v = 0: the device value must be exactly zero.

Memory: a factor is taken in row blocks (ROW_BLOCK rows); only the block is widened to longdouble, never the matrix."""
import numpy as np

LD = np.longdouble
# fail, do not skip: without an extended format there is no reference to hold the kernels to
assert np.finfo(LD).eps <= 1.1e-19, f"numpy.longdouble is not an extended format here (eps = {np.finfo(LD).eps})"

U = 2.0 ** -53          # unit roundoff of the device's doubles
U_LD = 2.0 ** -64       # ... of the 64-bit significand of numpy.longdouble
ROW_BLOCK = 512


def gamma(m, u=U):
    m = np.asarray(m, dtype=np.float64)
    return m * u / (1.0 - m * u)


def c_apply(n, dup, u=U):
    """c(n, d, u) of the module docstring: the error of one evaluation of z in unit roundoff u, relative to S"""
    g, gd = gamma(n, u), gamma(np.asarray(dup) + 1, u)
    return (2.0 * g + g * g) * (1.0 + gd) + gd


def c_unit_columns(n, dup, u=U):
    """the same for a unit-vector right-hand side evaluated with an exact first pass"""
    g, gd = gamma(n, u), gamma(np.asarray(dup) + 1, u)
    return g * (1.0 + gd) + gd


def multiplicity(l2gs, nV):
    dup = np.zeros(nV, dtype=np.int64)
    for l2g in l2gs:
        dup[np.asarray(l2g)] += 1
    return dup


def _dofs(l2g):
    return (3 * np.asarray(l2g, dtype=np.int64)[:, None] + np.arange(3)[None, :]).ravel()


def reference_apply(Xs, l2gs, nV, r):
    """z_ref and tol of the module docstring for the stored factors Xs[s] (n_s x n_s float64, vertex order l2gs[s]) and the right-hand
    side r of shape (nV, 3) -- or (m, nV, 3), m right-hand sides at once.  Returns arrays of r's shape: z_ref in longdouble (compare
    a device value with it in longdouble: rounding z_ref to float64 first would cost an error the tolerance does not hold), tol in
    float64."""
    r = np.asarray(r, dtype=np.float64)
    batch = r.ndim == 3
    R = (r if batch else r[None]).reshape(-1, 3 * nV).T.astype(LD)        # (3 nV, m)
    A = np.abs(R)
    Z = np.zeros_like(R)
    S = np.zeros_like(R)
    n = max(X.shape[0] for X in Xs)
    for X, l2g in zip(Xs, l2gs):
        d = _dofs(l2g)
        rs, ars = R[d], A[d]
        p = np.zeros_like(rs)
        sp = np.zeros_like(rs)
        for b0 in range(0, X.shape[0], ROW_BLOCK):
            Xb = X[b0:b0 + ROW_BLOCK]
            nz = np.flatnonzero((Xb != 0.0).any(axis=0))                  # (block-sparse: the columns the block holds at all)
            if nz.size == 0:
                continue
            Xw = Xb[:, nz].astype(LD)                                     # the one widened copy: a row block
            p[nz] += Xw.T @ (Xw @ rs[nz])
            Xw = np.abs(Xw)
            sp[nz] += Xw.T @ (Xw @ ars[nz])
        Z[d] += p
        S[d] += sp
    dup = np.repeat(multiplicity(l2gs, nV), 3)
    many = dup > 1
    Z[many] /= dup[many, None].astype(LD)
    S[many] /= dup[many, None].astype(LD)
    dupc = np.maximum(dup, 1)[:, None]
    c = c_apply(n, dupc) + c_apply(n, dupc, U_LD)
    tol = (c * S.astype(np.float64)) / (1.0 - gamma(2 * n + dupc + 1, U_LD))
    shape = r.shape if batch else (nV, 3)
    return Z.T.reshape(shape), tol.T.reshape(shape)


def reference_unit_columns(Xs, l2gs, nV, dofs):
    """The same for the unit vectors e_j, j in dofs (global scalar dofs 3 v + d), all at once in float64 BLAS: returns (Z, tol) of shape
    (len(dofs), nV, 3).  With r = e_j the first pass is exact (t = column j of X_s, products by 1.0 and sums of zeros), so the
    reference's own error is one second pass and the merge; it is ADDED to the tolerance (c_unit_columns at u)."""
    dofs = np.asarray(dofs, dtype=np.int64)
    m = dofs.size
    Z = np.zeros((3 * nV, m))
    S = np.zeros((3 * nV, m))
    n = max(X.shape[0] for X in Xs)
    for X, l2g in zip(Xs, l2gs):
        d = _dofs(l2g)
        loc = np.full(3 * nV, -1, dtype=np.int64)
        loc[d] = np.arange(d.size)
        cols = np.flatnonzero(loc[dofs] >= 0)                             # the right-hand sides that touch this subdomain
        if cols.size == 0:
            continue
        jl = loc[dofs[cols]]
        p = np.zeros((d.size, cols.size))
        sp = np.zeros((d.size, cols.size))
        for b0 in range(0, X.shape[0], 4 * ROW_BLOCK):
            Xb = X[b0:b0 + 4 * ROW_BLOCK]
            Tb = Xb[:, jl]                                                # t = X e_j, exactly
            p += Xb.T @ Tb
            sp += np.abs(Xb).T @ np.abs(Tb)
        Z[np.ix_(d, cols)] += p
        S[np.ix_(d, cols)] += sp
    dup = np.repeat(multiplicity(l2gs, nV), 3)
    many = dup > 1
    Z[many] /= dup[many, None]
    S[many] /= dup[many, None]
    dupc = np.maximum(dup, 1)[:, None]
    tol = (c_apply(n, dupc) + c_unit_columns(n, dupc)) * S / (1.0 - gamma(2 * n + dupc + 1))
    return Z.T.reshape(m, nV, 3), tol.T.reshape(m, nV, 3)
