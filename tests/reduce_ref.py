"""The arithmetic of include/mckpp_hip_reduce.h restated in numpy, for tests/test_reduce_*.py: plain loops over levels
and over the halves of an array, no call into the library and no np.sum.  Every numpy operation below is one rounded
fp64 operation per element.  The input is what window_record_fetch gives - x(npoints, levels kept) of one field and
operation of a record - with the positions that are rows marked."""
import numpy as np

NONE, SUM, AVERAGE, MIN, MAX = range(5)
W_LEVELS, W_POINTS = 1, 2


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def tree(t, op=SUM):
    """c: the terms padded to the next power of two, then halved: t[i] = t[i] (op) t[i + n]"""
    t = np.asarray(t, dtype=np.float64)
    n = 1
    while n < t.size:
        n *= 2
    pad = {MIN: np.inf, MAX: -np.inf}.get(op, 0.0)
    v = np.concatenate([t, np.full(n - t.size, pad)])
    if t.size == 0:
        return np.float64(0.0)
    while n > 1:
        n //= 2
        lo, hi = v[:n], v[n:2 * n]
        if op == MIN:
            v = np.where(hi < lo, hi, lo)
        elif op == MAX:
            v = np.where(hi > lo, hi, lo)
        else:
            v = lo + hi
    return v[0]


def staged(t, m):
    """the decomposition: the elements j, j + m, ... of each residue by the tree, then the m partials by the tree"""
    t = np.asarray(t, dtype=np.float64)
    n = 1
    while n < t.size:
        n *= 2
    v = np.concatenate([t, np.zeros(n - t.size)])
    if n <= m:
        return tree(v)
    return tree([tree(v[j::m]) for j in range(m)])


def left_to_right(t):
    """the other order, which the tests tell the tree from: s = t[0], then s = s + t[i] in ascending order (numpy's
    accumulate is that loop)"""
    t = np.asarray(t, dtype=np.float64)
    return np.add.accumulate(t)[-1] if t.size else np.float64(0.0)


def axis_reduce(x, op, wl, land):
    """b: x(nrows, nlev) down the levels in ascending order, wl the levels' weights or None"""
    nlev = x.shape[1]
    if op in (SUM, AVERAGE):
        a = x[:, 0] if wl is None else wl[0] * x[:, 0]
        for l in range(1, nlev):
            a = a + (x[:, l] if wl is None else wl[l] * x[:, l])
        if op == AVERAGE:
            w = np.float64(nlev)
            if wl is not None:
                w = np.float64(wl[0])
                for l in range(1, nlev):
                    w = w + wl[l]
            a = np.full(a.shape, land) if w == 0.0 else a / w
        return a
    a = x[:, 0]
    for l in range(1, nlev):
        a = np.where(x[:, l] < a, x[:, l], a) if op == MIN else np.where(x[:, l] > a, x[:, l], a)
    return a


def domain_terms(a, is_row, wp, op):
    """c: the term of every position - wp: the positions' point weights or None"""
    if op in (MIN, MAX):
        return np.where(is_row, a, np.inf if op == MIN else -np.inf)
    return np.where(is_row, a if wp is None else wp * a, 0.0)


def domain_reduce(a, is_row, wp, op, land):
    if not is_row.any():
        return np.float64(land)
    s = tree(domain_terms(a, is_row, wp, op), op)
    if op == AVERAGE:
        den = tree(np.where(is_row, 1.0 if wp is None else wp, 0.0))
        return np.float64(land) if den == 0.0 else s / den
    return s


def reduce_plane(x, is_row, axis_op, domain_op, wl, wp, land, seen=None):
    """x(npoints, nlev): the plane's levels; is_row(npoints); wl(nlev) / wp(npoints) or None.  The result as the array
    the library writes: (npoints), (nlev) or (1).  seen: a list that gets (tree sum, left-to-right sum) of every sum"""
    x = np.where(is_row[:, None], x, 0.0)   # (what a position that is no row holds is of no account)
    if axis_op != NONE:
        a = axis_reduce(x, axis_op, wl, land)
        if domain_op == NONE:
            return np.where(is_row, a, land)
        cols = [a]
    else:
        cols = [x[:, l] for l in range(x.shape[1])]
    if seen is not None and domain_op in (SUM, AVERAGE) and is_row.any():
        for c in cols:
            t = domain_terms(c, is_row, wp, domain_op)
            seen.append((tree(t), left_to_right(t)))
    return np.array([domain_reduce(c, is_row, wp, domain_op, land) for c in cols])
