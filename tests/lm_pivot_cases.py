"""Linear systems that make the LM solves (DmsaOptimizer.h:110-113: the explicit inverse by Gauss-Jordan with partial pivoting, then
step = (-alpha H^-1) g) SWAP rows and meet EQUAL |x| in the pivot column, and a plain model of the solve that counts both -- for
tests/test_lm_pivot_cases.py (CPU: the model against the oracle and the host solve) and tests/test_gpu_lm_pivots.py (the three device
solves against the model).

The forward-difference systems of tests/test_gpu_loop.py::_system / tests/nan_step_cases.py::regular_system are strongly diagonally
dominant: they make no swap and no tie at any size, so the pivot search, its tie rule ("first strict maximum from row k down" = "ties to
the smallest logical row") and the logical-to-physical row bookkeeping behind a swap are not exercised by them.  The families here:

  general       a dense standard-normal P x P matrix, not symmetric: a swap at most steps
  scaled_gram   J^T J + 1e-5 I for J of (4 P) x P with columns scaled by 10 ** U(-2, 2): symmetric like production systems, badly scaled
  paired_rows   `general` with P // 6 disjoint row pairs (a, b): row a scaled by U(1.5, 3), row b = -row a, and one column per pair among the
                last P // 6 where row b holds a value of its own.  Negation is exact, every pivot step does the same operation on a row and on
                its negative, so the two keep equal |x| in the pivot column until one of them is pivoted: ties AFTER earlier swaps
  planted_a_b   `general` with H[a, 0] = m, H[b, 0] = -m, m = 2 max |H[:, 0]|: a tie at step 0 between exactly rows a and b
  hadamard      a block diagonal of Sylvester-Hadamard blocks (one per binary digit of P), rows and columns permuted and their signs flipped,
                g of small integers, alpha = 0.25: dozens of ties, with and without the diagonal, many multipliers exactly zero.  Up to
                order 8 every operation is exact; from order 16 on a permuted block can have pivots that are no powers of two (8 / 3), so
                the larger sizes DO round, the tie order matters there like anywhere else, and the closed form H^-1 = H^T / n per block
                holds to a bound only (hadamard_closed_form_bound)
  hadamard8     the same from blocks of order 8 (and the binary digits of P % 8): every operation is exact at every P, every tie order gives
                the same bits, so it cannot tell a wrong tie-break from a right one -- it tells garbage from the closed form, bit for bit"""
import functools

import numpy as np

ALPHA = 0.2
LAMBDA = float(np.float32(1e-5))  # the reference's lambda_diag
STREAM_LANE_PAIR = 5              # rows r and r + 64: one lane and two register slots of the stream solve

# (P -> lm_stream values) of tests/nan_step_cases.py::SOLVE_TIERS plus 200; at 594 only `general` and `paired_rows` run (the panels alone)
TIERS = {6: (1,), 16: (1,), 17: (1,), 30: (1,), 64: (1,), 65: (1, 0), 128: (1, 0), 129: (1, 0), 186: (1, 0), 192: (1, 0), 193: (1,), 200: (1,), 594: (1,)}
LARGEST = 594


def model_step(H, g, alpha, tie="first", log=None):
    """invert_dense (oracle/dmsa_oracle.cpp) and the step product of lm_step as plain float64 operations on rows: partial pivoting by strict
    `>` from row k down, swap, x / d, x - f * s (skipped when f == 0.0), step[i] = sum_j (-alpha * inv[i][j]) * g[j] summed in order.  Every
    product and every difference is rounded on its own (numpy fuses nothing).
    -> (step, swaps, tie steps whose tied set includes the diagonal row, tie steps whose tied set does not); a tie step is a pivot step at which
    the largest |x| of the pivot column occurs in more than one candidate row.  tie="last" takes the LAST tied row instead of the first: it
    exists only to prove that a case can fail.  log: a list that receives (k, tied rows) of every tie step."""
    A = np.array(H, np.float64)
    P = A.shape[0]
    assert A.shape == (P, P) and tie in ("first", "last")
    g = np.asarray(g, np.float64)
    inv = np.eye(P)
    swaps = ties_diag = ties_off = 0
    with np.errstate(all="ignore"):
        for k in range(P):
            mag = np.abs(A[k:, k])
            piv = k
            if not np.isnan(mag[0]):  # (a NaN on the diagonal: nothing is > NaN, the diagonal stays)
                cand = np.where(np.isnan(mag), -1.0, mag)  # (a NaN is never > best)
                tied = np.flatnonzero(cand == cand.max())
                piv = k + int(tied[0] if tie == "first" else tied[-1])
                if tied.size > 1:
                    if tied[0] == 0:
                        ties_diag += 1
                    else:
                        ties_off += 1
                    if log is not None:
                        log.append((k, tuple(int(k + t) for t in tied)))
            if piv != k:
                swaps += 1
                A[[k, piv]] = A[[piv, k]]
                inv[[k, piv]] = inv[[piv, k]]
            d = A[k, k]
            A[k] = A[k] / d
            inv[k] = inv[k] / d
            f = A[:, k].copy()
            f[k] = 0.0
            rows = np.flatnonzero(f != 0.0)  # (f == 0.0 is skipped; a NaN multiplier is not)
            A[rows] = A[rows] - f[rows, None] * A[k][None, :]
            inv[rows] = inv[rows] - f[rows, None] * inv[k][None, :]
        terms = (-alpha * inv) * g[None, :]
        step = np.zeros(P)
        for j in range(P):
            step = step + terms[:, j]
    return step, swaps, ties_diag, ties_off


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the families --------------------------------------------------------------------------------------------------------------------
RESEED = {("general", 6): 2}  # six steps are few: the first draws swap at two of them, this one at half of them (the test counts)


def _seed(family, P):
    return [P, sum(family.encode())] + ([RESEED[family, P]] if (family, P) in RESEED else [])


def general(P, seed=None):
    rng = np.random.default_rng(_seed("general", P) if seed is None else seed)
    return rng.standard_normal((P, P)), rng.standard_normal(P)


def scaled_gram_jacobian(P):
    """-> (e0, J) with J of (4 P) x P"""
    rng = np.random.default_rng(_seed("scaled_gram", P))
    rows = 4 * P
    J = rng.standard_normal((rows, P)) * 10.0 ** rng.uniform(-2.0, 2.0, P)[None, :]
    return rng.uniform(0.5, 2.0, rows), J


def paired_rows(P):
    H, g = general(P, _seed("paired_rows", P))
    rng = np.random.default_rng(_seed("paired_rows_pairs", P))
    n = P // 6
    rows = rng.permutation(P)[: 2 * n].reshape(n, 2)
    for q, (a, b) in enumerate(rows):
        H[a] *= rng.uniform(1.5, 3.0)
        H[b] = -H[a]
        H[b, P - n + q] = rng.standard_normal()
    return H, g


def planted_pairs(P):
    """the row pairs (a, b) of the `planted` family that exist at P"""
    pairs = [(0, P - 1), (P - 2, P - 1), (63, 64), (127, 128), (STREAM_LANE_PAIR, STREAM_LANE_PAIR + 64), (1, 2)]
    out = []
    for a, b in pairs:
        if 0 <= a < b < P and (a, b) not in out:
            out.append((a, b))
    return out


def planted(P, a, b):
    H, g = general(P, _seed("planted", P) + [a, b])
    m = 2.0 * np.abs(H[:, 0]).max()
    H[a, 0], H[b, 0] = m, -m
    return H, g


def sylvester(n):
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    assert H.shape[0] == n
    return H


def hadamard_blocks(P, largest=None):
    """block sizes: one per binary digit of P; with `largest`, blocks of that size first and the binary digits of the rest"""
    sizes = []
    if largest is not None:
        sizes += [largest] * (P // largest)
        P -= largest * len(sizes)
    return sizes + [1 << bit for bit in reversed(range(P.bit_length())) if P & (1 << bit)]


def hadamard_ties_wanted(P):
    """(tie steps that include the diagonal, tie steps that do not) a Hadamard system of P rows must at least have: 1 and 8 from 30 rows
    on; a block of order n has at most n - 1 tie steps, so below 30 rows P // 4 stands for the 8"""
    return 1, (8 if P >= 30 else P // 4)


@functools.lru_cache(maxsize=None)
def hadamard(P, largest=None):
    """-> (H, g, closed-form inverse): H = R B C with B the block diagonal and R, C signed permutations, so H^-1 = C^T B^-1 R^T with
    B^-1 = blockdiag(H_n^T / n) -- every entry 0 or +-1/n, exact.  The permutation is the first of its seeded sequence whose system has the
    ties the family is for (hadamard_ties_wanted, counted by the model): a large block whose arithmetic rounds loses its ties early."""
    B, Binv = np.zeros((P, P)), np.zeros((P, P))
    at = 0
    for n in hadamard_blocks(P, largest):
        S = sylvester(n)
        B[at:at + n, at:at + n], Binv[at:at + n, at:at + n] = S, S.T / n
        at += n
    assert at == P
    for salt in range(32):
        rng = np.random.default_rng(_seed("hadamard", P) + [largest or 0, salt])
        pr, pc = rng.permutation(P), rng.permutation(P)
        sr, sc = rng.choice([-1.0, 1.0], P), rng.choice([-1.0, 1.0], P)
        H = sr[:, None] * B[pr][:, pc] * sc[None, :]          # H[i, j] = sr[i] B[pr[i], pc[j]] sc[j]
        Hinv = sc[:, None] * Binv[pc][:, pr] * sr[None, :]    # H^-1[j, i] = sc[j] Binv[pc[j], pr[i]] sr[i]
        g = rng.integers(-8, 9, P).astype(np.float64)
        _, _, ties_diag, ties_off = model_step(H, g, HADAMARD_ALPHA)
        if ties_diag >= hadamard_ties_wanted(P)[0] and ties_off >= hadamard_ties_wanted(P)[1]:
            return H, g, Hinv
    raise AssertionError(f"no permutation with the wanted ties at P = {P}")


HADAMARD_ALPHA = 0.25
SMALL_BLOCK = 8  # up to this order every pivot stays a power of two in whatever order the rows come (the CPU test confirms: exact, any tie order)


def hadamard_closed_form_step(P, largest=None):
    """step = -alpha H^-1 g from the closed form (+ 0.0: a sum that starts from 0.0 is never -0.0).  Every term is a small dyadic rational, so any
    summation order gives these bits."""
    _, g, Hinv = hadamard(P, largest)
    return -HADAMARD_ALPHA * (Hinv @ g) + 0.0


def hadamard_closed_form_bound(P):
    """How far a Gauss-Jordan step of `hadamard` may be from the closed form where its arithmetic is NOT exact.  From order 16 on the
    pivots of a row-permuted Sylvester matrix need not be powers of two (8 / 3 occurs), quotients round, and the step then carries the
    rounding of an elimination with partial pivoting: at most ~ P rho kappa u relative to the largest component (Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., theorem 9.5 with the growth factor rho <= n of a Hadamard block of order n and
    kappa = sqrt(n_max / n_min), the blocks being sqrt(n) times orthogonal), times 8 for the constants.  It tells garbage from a solve."""
    sizes = hadamard_blocks(P)
    n_max, n_min = max(sizes), min(sizes)
    return 8.0 * P * n_max * np.sqrt(n_max / n_min) * 2.0 ** -53 * np.abs(hadamard_closed_form_step(P)).max()


def case_names(P):
    """the cases run at P"""
    if P == LARGEST:
        return ["general", "paired_rows"]
    return ["general", "scaled_gram", "paired_rows", "hadamard", "hadamard8"] + [f"planted_{a}_{b}" for a, b in planted_pairs(P)]


@functools.lru_cache(maxsize=None)
def system(orc, name, P):
    """-> (H_damped [i, j], g, alpha) of case `name` at P.  scaled_gram takes its H and g from the oracle's own normal equations
    (orc.lm_step_from_jacobian), so that the step of that entry is the step of this system."""
    if name == "general":
        return general(P) + (ALPHA,)
    if name == "scaled_gram":
        e0, J = scaled_gram_jacobian(P)
        H, g, _ = orc.lm_step_from_jacobian(e0, J, LAMBDA, ALPHA)
        return H, g, ALPHA
    if name == "paired_rows":
        return paired_rows(P) + (ALPHA,)
    if name == "hadamard":
        return hadamard(P)[:2] + (HADAMARD_ALPHA,)
    if name == "hadamard8":
        return hadamard(P, SMALL_BLOCK)[:2] + (HADAMARD_ALPHA,)
    if name.startswith("planted_"):
        a, b = (int(x) for x in name.split("_")[1:])
        return planted(P, a, b) + (ALPHA,)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(orc, name, P):
    """-> (H, g, alpha, the model's step, swaps, ties with the diagonal, ties without, the tie log); computed once, never modified"""
    H, g, alpha = system(orc, name, P)
    log = []
    step, swaps, ties_diag, ties_off = model_step(H, g, alpha, log=log)
    for a in (H, g, step):
        a.setflags(write=False)
    return H, g, alpha, step, swaps, ties_diag, ties_off, tuple(log)
