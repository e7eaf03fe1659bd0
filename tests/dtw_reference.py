"""Dynamic time warping as include/taco_abi.h defines it, restated in float64 NumPy: frame cost, recurrence, tie rule, direction map and
path walk.  The tests hold taco_dtw and taco_dtw_path (csrc/taco_dtw.h) to this.

    cost_kind 0: c(i, j) = (1/D) * sum_d |a_id - b_jd|          cost_kind 1: c(i, j) = sqrt(sum_d (a_id - b_jd)^2)
    G(0,0) = 2 c(0,0);  G(i,0) = G(i-1,0) + c(i,0);  G(0,j) = G(0,j-1) + c(0,j)
    G(i,j) = min(G(i-1,j-1) + 2 c(i,j), G(i-1,j) + c(i,j), G(i,j-1) + c(i,j));   total = G(n-1,m-1);   dist = total / (n + m)

dir: 0 = from (i-1,j-1), 1 = from (i-1,j), 2 = from (i,j-1); the diagonal is tried first, then (i-1,j), then (i,j-1), a later candidate
replacing an earlier one under strict '<' only; border cells take their only predecessor and cell (0,0) is 0."""
import numpy as np


def clamp_len(length, T):
    """the device's rule for a length: into [1, T]; None = the full row"""
    return T if length is None else int(min(max(int(length), 1), T))


def frame_costs(a, b, cost_kind):
    """c [n, m] in float64, the sum over d taken in ascending order"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    D = a.shape[1]
    acc = np.zeros((a.shape[0], b.shape[0]))
    for d in range(D):
        diff = a[:, d][:, None] - b[:, d][None, :]
        acc = acc + (np.abs(diff) if cost_kind == 0 else diff * diff)
    return acc / D if cost_kind == 0 else np.sqrt(acc)


def dtw_loops(a, b, cost_kind=0):
    """The recurrence cell by cell, as the definition reads: a [n, D], b [m, D] (the used parts) -> (total, dist, dir [n, m] uint8,
    c [n, m]); total and dist are NaN when an element is not finite (dir is then unspecified)."""
    if cost_kind not in (0, 1):
        raise ValueError("cost_kind must be 0 or 1")
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n, m = a.shape[0], b.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        c = frame_costs(a, b, cost_kind)
    G = np.zeros((n, m))
    dr = np.zeros((n, m), np.uint8)
    for i in range(n):
        for j in range(m):
            cij = c[i, j]
            if i == 0 and j == 0:
                G[i, j], dr[i, j] = 2 * cij, 0
            elif j == 0:
                G[i, j], dr[i, j] = G[i - 1, 0] + cij, 1
            elif i == 0:
                G[i, j], dr[i, j] = G[0, j - 1] + cij, 2
            else:
                best, k = G[i - 1, j - 1] + 2 * cij, 0
                up, left = G[i - 1, j] + cij, G[i, j - 1] + cij
                if up < best:
                    best, k = up, 1
                if left < best:
                    best, k = left, 2
                G[i, j], dr[i, j] = best, k
    total = G[n - 1, m - 1]
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        total = np.nan
    return total, total / (n + m), dr, c


def dtw(a, b, cost_kind=0):
    """dtw_loops one anti-diagonal at a time (the cells of a diagonal depend on the two diagonals before only): the same operations on
    the same operands, so the same bits, at NumPy's speed.  A missing predecessor is +inf, which no finite candidate fails to beat under
    '<', so border cells take their only predecessor; the cell before (0,0) counts as 0."""
    if cost_kind not in (0, 1):
        raise ValueError("cost_kind must be 0 or 1")
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n, m = a.shape[0], b.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        c = frame_costs(a, b, cost_kind)
        Gp = np.full((n + 1, m + 1), np.inf)          # Gp[i + 1, j + 1] = G(i, j)
        Gp[0, 0] = 0.0
        dr = np.zeros((n, m), np.uint8)
        for s in range(n + m - 1):
            i = np.arange(max(0, s - m + 1), min(n - 1, s) + 1)
            j = s - i
            cc = c[i, j]
            best = Gp[i, j] + 2 * cc
            k = np.zeros(len(i), np.uint8)
            up, left = Gp[i, j + 1] + cc, Gp[i + 1, j] + cc
            t = up < best
            best, k = np.where(t, up, best), np.where(t, np.uint8(1), k)
            t = left < best
            best, k = np.where(t, left, best), np.where(t, np.uint8(2), k)
            Gp[i + 1, j + 1], dr[i, j] = best, k
    total = Gp[n, m]
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        total = np.nan
    return total, total / (n + m), dr, c


def walk(dr, n, m):
    """The warping path from a direction map, ascending from (0,0) to (n-1,m-1), [L, 2] int32.  Any byte content is walked safely: a byte
    above 2 counts as 0, in row 0 the move is (0, j-1), in column 0 (i-1, 0); at most n + m - 1 entries."""
    i, j = n - 1, m - 1
    out = []
    for _ in range(n + m - 1):
        out.append((i, j))
        if i == 0 and j == 0:
            break
        d = int(dr[i, j])
        if d > 2:
            d = 0
        if i == 0:
            d = 2
        elif j == 0:
            d = 1
        if d != 2:
            i -= 1
        if d != 1:
            j -= 1
    return np.array(out[::-1], np.int32).reshape(-1, 2)


def path_is_valid(path, n, m):
    """starts at (0,0), ends at (n-1,m-1), every step is one of (1,1), (1,0), (0,1)"""
    path = np.asarray(path, np.int64)
    if len(path) < 1 or tuple(path[0]) != (0, 0) or tuple(path[-1]) != (n - 1, m - 1):
        return False
    steps = set(map(tuple, np.diff(path, axis=0)))
    return steps <= {(1, 1), (1, 0), (0, 1)}


def path_cost(path, c):
    """the weighted cost along a path in float64: 2 c at (0,0) and after a diagonal step, c after the other two"""
    path = np.asarray(path, np.int64)
    w = np.where((np.diff(path, axis=0) == 1).all(axis=1), 2.0, 1.0)
    tot = 2 * c[0, 0]
    for t in w * c[path[1:, 0], path[1:, 1]]:          # in path order, as the recurrence adds them
        tot = tot + t
    return tot


def dtw_batch(A, Bm, len_a=None, len_b=None, cost_kind=0):
    """Rectangles [B, Ta, D], [B, Tb, D] with lengths (clamped as the device clamps them) -> per pair a dict(n, m, total, dist, dir, c,
    path)."""
    out = []
    for p in range(A.shape[0]):
        n = clamp_len(None if len_a is None else len_a[p], A.shape[1])
        m = clamp_len(None if len_b is None else len_b[p], Bm.shape[1])
        total, dist, dr, c = dtw(A[p, :n], Bm[p, :m], cost_kind)
        out.append(dict(n=n, m=m, total=total, dist=dist, dir=dr, c=c, path=walk(dr, n, m)))
    return out
