"""An order-independent check of the normal equations H = J^T J (+ lambda I), g = J^T e0 of the LM step (DmsaOptimizer.h:96-110).

J is built in float64 exactly as the kernels build it (ne_col / k_jacobian_columns: (1/h) * (e_k - e0)), so both sides multiply the same
numbers; the products are then summed in long double (64-bit mantissa) or, where long double is only double, with math.fsum.  Any float64
summation of n terms, in any order and with or without fused multiply-adds, stays within gamma_n * |J|^T |J| of the exact dot product
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 3.5): a wrong tile, mirror, padding column or row block misses it by
orders of magnitude, while the blocked order of the library and of the oracle both pass.
"""
import math
import os

import numpy as np

U = 2.0 ** -53


def gamma(n: int, u: float = U) -> float:
    return n * u / (1.0 - n * u)


def jacobian(e0, e_batch, h):
    """(rows x P) columns (1/h) * (e_k - e0) in float64, the kernels' operation sequence (inv_h = 1.0 / h on the host)."""
    e0 = np.asarray(e0, np.float64)
    eb = np.asarray(e_batch, np.float64)
    inv_h = 1.0 / float(h)
    return np.ascontiguousarray((inv_h * (eb - e0[None, :])).T)


def _exact_products(A, B):
    """A^T B with (nearly) exact sums: long double where it has a 64-bit mantissa (the oracle's threaded C loop: numpy's long double
    matmul manages ~10^8 products per second, minutes at P ~ 1000), else math.fsum of the float64 products (exact for products that do
    not round, which float64 * float64 may; the rounding of each product is then covered by the u of gamma)."""
    if np.finfo(np.longdouble).nmant >= 63:
        from oracle import oracle_py

        threads = min(16, int(os.environ.get("OMP_NUM_THREADS", "16")))
        return oracle_py.gram_long_double(A, B, threads), gamma(A.shape[0], 2.0 ** -64)
    out = np.empty((A.shape[1], B.shape[1]), np.float64)
    for i in range(A.shape[1]):
        for j in range(B.shape[1]):
            out[i, j] = math.fsum((A[:, i] * B[:, j]).tolist())
    return out, 2.0 * U  # the product roundings + the final rounding of fsum


def reference(e0, e_batch, h):
    """-> J, H_hat = J^T J, g_hat = J^T e0 (long double), and the elementwise bounds of a float64 evaluation of H and g."""
    e0 = np.asarray(e0, np.float64)
    J = jacobian(e0, e_batch, h)
    rows = J.shape[0]
    Je = np.concatenate([J, e0[:, None]], axis=1)
    Hx, ref_err = _exact_products(J, Je)
    H_hat, g_hat = Hx[:, :-1], Hx[:, -1]
    absJ = np.abs(J)
    Ax, _ = _exact_products(absJ, np.concatenate([absJ, np.abs(e0)[:, None]], axis=1))
    scale = gamma(rows) + ref_err  # the float64 sums + what the reference itself may be off by
    return J, H_hat, g_hat, scale * Ax[:, :-1], scale * Ax[:, -1]


def check(H, g, lam, e0, e_batch, h):
    """Assert that H (damped by lam) and g are a float64 evaluation of J^T J + lam I and J^T e0 within the forward-error bound.
    Returns the largest ratio |error| / bound seen (<= 1 passes)."""
    H = np.asarray(H, np.float64)
    g = np.asarray(g, np.float64)
    P = H.shape[0]
    J, H_hat, g_hat, bH, bg = reference(e0, e_batch, h)
    assert J.shape[1] == P and g.shape == (P,)
    lam = float(lam)
    # the diagonal's lam is added to the float64 sum in one more rounding: at most u |H_ii|
    bH = bH + np.diag(U * np.abs(np.diag(H)))
    errH = np.abs(H.astype(np.longdouble) - np.longdouble(lam) * np.eye(P, dtype=np.longdouble) - H_hat)
    errg = np.abs(g.astype(np.longdouble) - g_hat)
    bad = np.argwhere(errH > bH)
    assert bad.size == 0, f"H outside the fp64 bound at {bad[:5].tolist()} (of {len(bad)}): err {errH[tuple(bad[0])]} > bound {bH[tuple(bad[0])]}"
    badg = np.flatnonzero(errg > bg)
    assert badg.size == 0, f"g outside the fp64 bound at {badg[:5].tolist()}: err {errg[badg[0]]} > bound {bg[badg[0]]}"
    with np.errstate(divide="ignore", invalid="ignore"):
        rH = np.where(bH > 0, errH / bH, np.where(errH > 0, np.inf, 0.0))
        rg = np.where(bg > 0, errg / bg, np.where(errg > 0, np.inf, 0.0))
    return float(max(rH.max(), rg.max()))
