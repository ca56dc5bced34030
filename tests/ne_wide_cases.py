"""The summation order of the normal equations and of the line search's squared sums, restated for tests/test_ne_wide_cases.py (CPU: the
oracle's export against the exact chain) and tests/test_gpu_ne_wide.py (k_jacobian_columns + k_normal_eq_mfma + k_normal_eq_reduce above 64
parameters, and k_squared_sums_blocked, on caller data).

The rule (oracle/dmsa_oracle.cpp: reduction_block_rows, blocked_dot): rows are cut into consecutive blocks, every block is summed row by row
from 0.0, the block sums are added in block order from 0.0.  Up to 64 parameters a block has 256 rows and every step is a rounded product and
a rounded sum; above, a block has max(256, ceil(ceil(rows / 32) / 32) * 32) rows (at most 32 blocks) and every step is ONE fused
multiply-add, s = fma(x[r], y[r], s) -- what a chain of v_mfma_f64_16x16x4_f64 computes.

The fused chain is restated exactly: fma(a, b, s) = float(Fraction(a) * Fraction(b) + Fraction(s)), one correct rounding of the exact value,
denormals included; infinities and NaNs are handled apart.  That is slow, so it runs on a SAMPLE of the matrix (sample_pairs); the whole matrix
is compared with the oracle's export of blocked_dot, which the CPU test pins to the chain on the same sample."""
import functools
import math
from fractions import Fraction

import numpy as np


def reduction_block_rows(rows, P):
    rs = 256
    if P > 64:
        want = (rows + 31) // 32
        rs = max(256, ((want + 31) // 32) * 32)
    return rs


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def columns(E, h, formed):
    """[J | e0] as the kernels form it: column k = inv_h * (E[k + 1] - E[0]), column P = E[0]; formed: E[k + 1] and E[0] as they are"""
    with np.errstate(all="ignore"):
        if formed:
            return np.concatenate([E[1:], E[:1]])
        inv_h = 1.0 / h
        return np.concatenate([inv_h * (E[1:] - E[0]), E[:1]])


def formed_batch(E, h):
    """the batch that holds the columns of `E` already: the same [J | e0] through formed = 1"""
    A = columns(E, h, False)
    return np.concatenate([A[-1:], A[:-1]])


# ---- the unfused order, in numpy ---------------------------------------------------------------------------------------------------------
def unfused_gram(A, rs):
    """Hp[i, j] of the columns A (n1, rows): per block of rs rows c = c + a * b row by row, the block sums added in block order"""
    with np.errstate(all="ignore"):
        n1, rows = A.shape
        Hp = np.zeros((n1, n1))
        for r0 in range(0, rows, rs):
            c = np.zeros((n1, n1))
            for r in range(r0, min(rows, r0 + rs)):
                c = c + A[:, r, None] * A[None, :, r]
            Hp = Hp + c
    return Hp


def unfused_squares(E, rs):
    with np.errstate(all="ignore"):
        B, rows = E.shape
        out = np.zeros(B)
        for r0 in range(0, rows, rs):
            c = np.zeros(B)
            for r in range(r0, min(rows, r0 + rs)):
                c = c + E[:, r] * E[:, r]
            out = out + c
    return out


# ---- the fused order, exactly ------------------------------------------------------------------------------------------------------------
def fma_exact(a, b, s):
    """fma(a, b, s) by its definition: the exact a * b + s, rounded once"""
    a, b, s = float(a), float(b), float(s)
    if not (math.isfinite(a) and math.isfinite(b)):
        return a * b + s  # the product is an infinity or a NaN as it stands: nothing rounds
    if not math.isfinite(s):
        return s
    exact = Fraction(a) * Fraction(b) + Fraction(s)
    if exact == 0:
        return a * b + s  # the sign of an exact zero: (+-0) + (+-0), nothing rounds
    try:
        return float(exact)
    except OverflowError:
        return math.inf if exact > 0 else -math.inf


def _dyadic(v):
    """a finite v as (n, k): v = n / 2 ** k"""
    n, d = v.as_integer_ratio()
    return n, d.bit_length() - 1


def _operands(x):
    """per element (n, k), or None where the element is not finite"""
    return [_dyadic(v) if math.isfinite(v) else None for v in x.tolist()]


def fused_chain(x, y, ox=None, oy=None):
    """s = fma(x[r], y[r], s) over the rows, from 0.0 -- fma_exact step by step, on integers: every finite double is n / 2 ** k, so the exact
    a * b + s is an integer over a power of two, and int / int is correctly rounded like float(Fraction) (which IS int / int).  ox, oy: the
    _operands of x and y, if the caller has them."""
    ox = _operands(x) if ox is None else ox
    oy = _operands(y) if oy is None else oy
    xs, ys = x.tolist(), y.tolist()
    s, sn, sk = 0.0, 0, 0
    for r in range(len(xs)):
        a, b = ox[r], oy[r]
        if a is None or b is None or sn is None:
            s = fma_exact(xs[r], ys[r], s)
        else:
            pk = a[1] + b[1]
            if pk >= sk:
                num, k = a[0] * b[0] + (sn << (pk - sk)), pk
            else:
                num, k = ((a[0] * b[0]) << (sk - pk)) + sn, sk
            if num == 0:
                s = xs[r] * ys[r] + s
            else:
                try:
                    s = num / (1 << k)
                except OverflowError:
                    s = math.inf if num > 0 else -math.inf
        if math.isfinite(s):
            sn, sk = _dyadic(s)
        else:
            sn = None
    return s


def fused_dot(x, y, rs, ox=None, oy=None):
    """blocked_dot with the fused rule: the chains of the blocks of rs rows, added in block order"""
    with np.errstate(all="ignore"):
        total = np.float64(0.0)
        for r0 in range(0, len(x), rs):
            sl = slice(r0, min(len(x), r0 + rs))
            total = total + np.float64(fused_chain(x[sl], y[sl], None if ox is None else ox[sl], None if oy is None else oy[sl]))
    return float(total)


def sample_pairs(P):
    """the elements (i, j), i <= j, the exact chain runs on: the whole e0 row and column, the diagonal, and every (i, j) with i, j in
    {0, 15, 16, 31, 32, ..., P} -- every 16 x 16 wave quarter and every tile edge"""
    grid = sorted({0, P} | {c for m in range(1, P // 16 + 2) for c in (16 * m - 1, 16 * m) if c <= P})
    pairs = {(i, P) for i in range(P + 1)} | {(i, i) for i in range(P + 1)} | {(i, j) for i in grid for j in grid if i <= j}
    return sorted(pairs)


def fused_sample(A, P):
    """{(i, j): the fused blocked sum of columns i and j of A (n1, rows)} on sample_pairs(P)"""
    rs = reduction_block_rows(A.shape[1], P)
    ops = [_operands(col) for col in A]
    return {(i, j): fused_dot(A[i], A[j], rs, ops[i], ops[j]) for i, j in sample_pairs(P)}


def fused_squares(E, P):
    rs = reduction_block_rows(E.shape[1], P)
    return np.array([fused_dot(e, e, rs) for e in E])


def same_bits_or_nan(got, ref, what):
    """the bit patterns wherever the reference is not a NaN, and the NaN positions: which NaN an operation generates (inf - inf, 0 * inf) is
    the platform's choice, no property of the summation"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(bits(got)[~nan], bits(ref)[~nan]), (what, np.argwhere(bits(got) != bits(ref))[:5].tolist())


def check_sample(Hp, sample, what):
    """Hp[i, j] and Hp[j, i] against the chain of (i, j): a * b and b * a round alike (NaN signs aside, and those are not compared)"""
    for (i, j), ref in sample.items():
        for got in (Hp[i, j], Hp[j, i]):
            if math.isnan(ref):
                assert math.isnan(got), (what, i, j)
            else:
                assert bits(got) == bits(ref), (what, i, j, float(got), ref)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
H_STEP = 1e-3
NE_PARAMS = (65, 95, 96, 127, 128, 200)       # nt = 3 with a 2-column and with a full last tile, e0 alone in a tile, nt = 4 full, nt = 5
NE_ROWS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)
NE_PARAMS_LONG = (65, 96, 128)
NE_ROWS_LONG = (3840, 4096, 4097, 8192, 8193, 9216, 9217)  # 15, 16, 17, 32, 29, 32, 29 blocks of 256, 256, 256, 256, 288, 288, 320 rows
NE_CASES = [(P, rows) for P in NE_PARAMS for rows in NE_ROWS] + [(P, rows) for P in NE_PARAMS_LONG for rows in NE_ROWS_LONG]
NE_BOUND_ROWS = 257                            # the case per P that also goes through tests/ne_bound.py

SPECIAL = {"nan": np.nan, "inf": np.inf, "minus_zero": -0.0, "denormal": 5e-324 * 12345, "tiny": 1e-160}
SPECIAL_SHAPES = ((65, 257), (96, 320), (128, 513))

SQ_EVALS, SQ_PARAMS = (1, 9, 33), (64, 65)
SQ_ROWS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
SQ_ROWS_LONG = (32768, 32769, 65537)           # P = 65, B = 2: one, two and three 1024-row chunks per block
SQ_CASES = [(B, P, rows) for P in SQ_PARAMS for B in SQ_EVALS for rows in SQ_ROWS] + [(2, 65, rows) for rows in SQ_ROWS_LONG]


def batch(P, rows, seed=None):
    """a residual batch E (P + 1, rows)"""
    return np.random.default_rng([P, rows] if seed is None else seed).standard_normal((P + 1, rows))


def special_batch(P, rows, name, where):
    """tests/test_gpu_ne_triangle.py's special values above 64 parameters: one entry of e0 or of column P - 31 (and a whole evaluation of
    -0.0 beside a -0.0); `tiny` scales the WHOLE evaluation by 1e-160, so that every product of two of its entries is a
    denormal and so is their sum"""
    E = batch(P, rows, [P, rows, 7])
    at = 0 if where == "e0" else P - 30
    if name == "tiny":
        E[at] *= SPECIAL[name]
        return E
    E[at, rows - 2] = SPECIAL[name]
    if name == "minus_zero":
        E[1 if where == "e0" else 2] = -0.0
    return E


@functools.lru_cache(maxsize=None)
def squares_input(B, rows, kind):
    """E (B, rows) for the squared sums.  random: standard normal.  cancellation: 1 +- k 2^-27, whose square 1 +- k 2^-26 + k^2 2^-54 needs more
    than 53 bits: the unfused rule drops 2^-54 of every square before it adds, the fused rule adds the exact square.  Whether that shows in
    the rounded sum is a matter of chance row by row, so the input is the first draw of its seeded sequence on which the two rules (at 65
    parameters) give different sums in at least one evaluation; one row cannot differ (one square, rounded once either way)."""
    for draw in range(64):
        rng = np.random.default_rng([B, rows, len(kind), draw])
        if kind == "random":
            E = rng.standard_normal((B, rows))
        else:
            assert kind == "cancellation"
            E = 1.0 + rng.integers(1, 1 << 12, (B, rows)) * rng.choice([-1, 1], (B, rows)) * 2.0 ** -27
        if kind == "random" or rows == 1 or not np.array_equal(bits(fused_squares(E, 65)), bits(unfused_squares(E, reduction_block_rows(rows, 65)))):
            E.setflags(write=False)
            return E
    raise AssertionError((B, rows, kind))
