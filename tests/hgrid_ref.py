"""The arithmetic of include/mckpp_hip_hgrid.h restated in numpy - a loop over the entry position, vectorised over the
rows, every product and every sum one rounded fp64 operation as numpy's element-wise ones are - and the weight tables
the tests use, built from fixed seeds.  A table is the CSR triple (ptr int64, idx int32, w float64).  No pytest, no GPU."""
import numpy as np

LAND = 1e20
LENGTHS = (0, 1, 4, 9, 70)      # row lengths of the general tables: 70 is more than a slice has rows
NORMS = ("none", "used")


def apply(table, x, nrows, used=None, norm=None, fill=True, land_value=LAND, out=None):
    """One level through `table`.  used: per source index, whether entries that read it are used (None: all).  norm
    None: the in direction, the plain sum (0.0 for a row without a used entry); "none" / "used": the out direction, where
    a row without a used entry - or, under "used", with the used weights summing to 0.0 - gets land_value (fill) or
    keeps what `out` held."""
    ptr, idx, w = table
    x = np.asarray(x, dtype=np.float64)
    lens = np.diff(ptr)
    a, d, cnt = np.zeros(nrows), np.zeros(nrows), np.zeros(nrows, dtype=np.int64)
    for k in range(int(lens.max(initial=0))):
        rows = np.nonzero(lens > k)[0]
        e = ptr[rows] + k
        i = idx[e]
        if used is not None:
            m = np.asarray(used)[i] != 0
            rows, e, i = rows[m], e[m], i[m]
        wx = w[e] * x[i]
        first = cnt[rows] == 0
        a[rows] = np.where(first, wx, a[rows] + wx)       # the first used entry assigns
        d[rows] = np.where(first, w[e], d[rows] + w[e])
        cnt[rows] += 1
    if norm is None:
        return a
    assert norm in NORMS
    some = cnt > 0
    if norm == "used":
        some &= d != 0.0
    if out is None and not fill:
        raise ValueError("keep needs what out held")
    res = np.full(nrows, land_value) if fill else np.array(out, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = a / d if norm == "used" else a
    res[some] = v[some]
    return res


def csr(rows):
    """the CSR triple of a list of rows, each a list of (index, weight)"""
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.array([i for r in rows for i, _ in r], dtype=np.int32)
    w = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return ptr, idx, w


def grids(npts):
    """the two caller grids of a case: fewer points than a wave has lanes, and about 1.3 npts, no multiple of 64"""
    big = int(1.3 * npts) + 1
    while big % 64 == 0:
        big += 1
    return 37, big


def identity_in(npts, n, seed):
    """(table, perm): model point p reads caller point perm[p] with weight 1.0 - a permutation of the caller grid"""
    assert n >= npts
    perm = np.random.default_rng(seed).permutation(n)[:npts]
    return csr([[(int(perm[p]), 1.0)] for p in range(npts)]), perm


def through(perm, n, x, junk=3e33):
    """x(..., npts) on the caller grid of identity_in: x[p] at perm[p], a value nothing may read elsewhere"""
    out = np.full(x.shape[:-1] + (n,), junk)
    out[..., perm] = x
    return out


def _row(rng, length, nsrc):
    """`length` entries: indices with repetitions, weights of both signs"""
    idx = rng.integers(0, nsrc, size=length)
    w = rng.uniform(-0.25, 1.0, size=length) / max(length, 1)     # (a row's weights sum to less than 1: mild values)
    return [(int(i), float(v)) for i, v in zip(idx, w)]


def general_in(npts, n, ocean, seed):
    """Caller -> model: every row length of LENGTHS; the empty rows at land points only.  Row 1 - an ocean point of
    every case - has 70 entries, between short rows in the first slice."""
    rng = np.random.default_rng(seed)
    rows = []
    for p in range(npts):
        length = int(rng.choice(LENGTHS if not ocean[p] else LENGTHS[1:], p=None))
        if p == 1:
            length = 70
        elif p < 8:
            length = min(length, 4)
        rows.append(_row(rng, length, n))
    return csr(rows)


def general_out(n, npts, ocean, seed):
    """Model -> caller: every row length of LENGTHS, and by construction row 0 empty, row 1 of 70 entries between short
    rows, row 2 of land entries only, row 3 of one land and three ocean entries, row 4 of two ocean entries whose
    weights sum to 0.0 between two land entries, row 5 a lone ocean entry of weight -1.0."""
    rng = np.random.default_rng(seed)
    land, sea = np.nonzero(np.asarray(ocean) == 0)[0], np.nonzero(ocean)[0]
    assert land.size and sea.size >= 4
    rows = []
    for j in range(n):
        length = int(rng.choice(LENGTHS))
        if j < 8:
            length = min(length, 4)
        rows.append(_row(rng, length, npts))
    rows[0] = []
    rows[1] = _row(rng, 70, npts)
    rows[2] = [(int(land[k % land.size]), 0.5) for k in range(4)]
    rows[3] = [(int(sea[0]), 0.25), (int(land[0]), 0.5), (int(sea[1]), 0.125), (int(sea[2]), 0.125)]
    rows[4] = [(int(sea[1]), 0.5), (int(land[0]), 0.375), (int(sea[3]), -0.5), (int(land[-1]), 0.25)]
    rows[5] = [(int(sea[2]), -1.0)]
    return csr(rows)


def row_kinds(table, ocean):
    """per row of an out table: 0 no entry, 1 land entries only, 2 land and ocean entries, 3 ocean entries only"""
    ptr, idx, _ = table
    kinds = np.zeros(ptr.size - 1, dtype=np.int64)
    for r in range(kinds.size):
        o = np.asarray(ocean)[idx[ptr[r]:ptr[r + 1]]] != 0
        kinds[r] = 0 if o.size == 0 else 1 if not o.any() else 3 if o.all() else 2
    return kinds
