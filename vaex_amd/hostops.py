"""Host-side finishing of large results (a groupby's 1e6-group label column, a mean's
division) in page-locked, already-faulted memory, split over a few threads: numpy releases
the GIL inside ufunc loops, and a fresh 8 MB output costs ~2000 page faults on first touch.
Results are bit-identical to the single numpy call (element-wise operations)."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib

MIN_SPLIT = 1 << 18  # below this a single call is cheaper than the hand-off
_pool = None
_pool_lock = threading.Lock()


def _threads():
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        n = os.cpu_count() or 1
    return max(1, min(8, n, int(os.environ.get("OMP_NUM_THREADS", n))))


def _get_pool():
    global _pool
    with _pool_lock:
        if _pool is None:
            _pool = ThreadPoolExecutor(_threads(), thread_name_prefix="vaex_amd_host")
    return _pool


def submit(fn, *args):
    """fn(*args) on the host pool (a Future): host work overlapped with a GPU pass, which
    releases the GIL while the library waits on the device."""
    return _get_pool().submit(fn, *args)


def _run(fn, n, min_split=MIN_SPLIT):
    """fn(i0, i1) over [0, n) in chunks, on the pool when n is large."""
    k = min(_threads(), max(1, n // min_split))
    if k == 1:
        fn(0, n)
        return
    pool = _get_pool()
    b = [n * i // k for i in range(k + 1)]
    for f in [pool.submit(fn, b[i], b[i + 1]) for i in range(k)]:
        f.result()


def _empty(n, dtype):
    """Page-locked output from the library's block cache (faulted in already); plain memory
    where the runtime has none to give (no device: the CPU-only tests)."""
    try:
        return _lib.pinned_empty(n, dtype)
    except _lib.HipError:
        return np.empty(n, dtype)


def true_divide(a, b):
    """a / b (numpy true division, divide / invalid ignored) for 1-d arrays."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim != 1 or b.shape != a.shape or len(a) < MIN_SPLIT:
        with np.errstate(divide="ignore", invalid="ignore"):
            return a / b
    with np.errstate(divide="ignore", invalid="ignore"):
        out = _empty(len(a), np.true_divide(a[:1], b[:1]).dtype)

    def part(i0, i1):
        with np.errstate(divide="ignore", invalid="ignore"):
            np.true_divide(a[i0:i1], b[i0:i1], out=out[i0:i1])

    _run(part, len(a))
    return out


def arange(vmin, n, dtype, threads=True):
    """vmin .. vmin + n - 1 in `dtype` (every value representable in it).  threads=False: on
    the calling thread only (a job already running on the pool must not wait on it)."""
    dtype = np.dtype(dtype)
    if n < MIN_SPLIT:
        return np.arange(vmin, vmin + n, dtype=dtype)
    out = _empty(n, dtype)

    def part(i0, i1):
        out[i0:i1] = np.arange(vmin + i0, vmin + i1, dtype=dtype)

    if threads:
        _run(part, n)
    else:
        part(0, n)
    return out


def astype(a, dtype):
    """a.astype(dtype, copy=False) for a 1-d array (a C cast, element-wise)."""
    a, dtype = np.asarray(a), np.dtype(dtype)
    if a.dtype == dtype or a.ndim != 1 or len(a) < MIN_SPLIT:
        return a.astype(dtype, copy=False)
    out = _empty(len(a), dtype)

    def part(i0, i1):
        out[i0:i1] = a[i0:i1]

    _run(part, len(a))
    return out


def take(a, idx):
    """a[idx] for a 1-d array and an int64 index array (in range)."""
    return take_columns([a], idx)[0]


def take_columns(cols, idx):
    """[c[idx] for c in cols] (1-d arrays, int64 indices in range): one call of the library's
    host gather over the host threads, each thread one index range of every column (numpy's
    take holds the interpreter lock)."""
    import ctypes
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    cols = [np.asarray(c) for c in cols]
    fast = [c.ndim == 1 and c.dtype.itemsize in (1, 2, 4, 8) and not c.dtype.hasobject for c in cols]
    out = [None] * len(cols)
    if len(idx) >= MIN_SPLIT // 8:
        todo = [i for i, f in enumerate(fast) if f]
        srcs = [np.ascontiguousarray(cols[i]) for i in todo]
        dsts = [_empty(len(idx), s.dtype) for s in srcs]
        if todo:
            k = len(todo)
            _lib.call("vh_host_take", k, (ctypes.c_void_p * k)(*[d.ctypes.data for d in dsts]),
                      (ctypes.c_void_p * k)(*[s.ctypes.data for s in srcs]), (ctypes.c_int * k)(*[s.dtype.itemsize for s in srcs]),
                      idx.ctypes.data, len(idx), _threads())
        for i, d in zip(todo, dsts):
            out[i] = d
    for i, c in enumerate(cols):
        if out[i] is None:
            out[i] = np.take(c, idx)
    return out


def variance(sum_moment, sums, counts):
    """agg.py:207-213's finish, element-wise in the same operations (bit-identical to the
    numpy expression): mean = sum / count, m2 / count - mean ** 2, over the host threads (the
    inputs may be strided views of the grids' host images; the work is split along the last
    axis)."""
    sm = np.asarray(sum_moment, dtype=np.float64)
    s = np.asarray(sums, dtype=np.float64)
    c = np.asarray(counts)
    if sm.shape != s.shape or s.shape != c.shape or sm.size < MIN_SPLIT or sm.ndim == 0:
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = s / c
            return sm / c - mean ** 2
    order = "F" if sm.ndim > 1 and not sm.flags.c_contiguous else "C"
    out = np.empty(sm.shape, np.float64, order=order)

    def part(i0, i1):
        sl = (Ellipsis, slice(i0, i1))
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = s[sl] / c[sl]
            np.subtract(sm[sl] / c[sl], mean * mean, out=out[sl])

    last = sm.shape[-1]
    if last >= 8:
        _run(part, last, max(1, last // 8))
    else:
        part(0, last)
    return out


def minmax(a):
    """(a.min(), a.max()) of a non-empty 1-d integer array."""
    a = np.asarray(a)
    if a.ndim != 1 or len(a) < MIN_SPLIT:
        return a.min(), a.max()
    res = {}

    def part(i0, i1):
        res[i0] = (a[i0:i1].min(), a[i0:i1].max())

    _run(part, len(a))
    return min(v[0] for v in res.values()), max(v[1] for v in res.values())


def occupancy(a):
    """(nonzero count, first nonzero index, last nonzero index) of a 1-d array ((0, -1, -1)
    when all are zero): count_nonzero per chunk on the host threads; the first / last index
    is searched only inside chunks that are not fully occupied (a dense groupby's count grid
    usually is)."""
    a = np.asarray(a)
    n = len(a)
    res = {}

    def part(i0, i1):
        c = a[i0:i1]
        nz = int(np.count_nonzero(c))
        if nz == 0:
            res[i0] = (0, -1, -1)
        elif nz == i1 - i0:
            res[i0] = (nz, i0, i1 - 1)
        else:
            idx = np.flatnonzero(c)
            res[i0] = (nz, i0 + int(idx[0]), i0 + int(idx[-1]))

    if n:
        _run(part, n, MIN_SPLIT // 8)  # a streaming count: every thread's memory bandwidth helps
    parts = [res[k] for k in sorted(res)]
    nnz = sum(p[0] for p in parts)
    firsts = [p[1] for p in parts if p[0]]
    lasts = [p[2] for p in parts if p[0]]
    return nnz, (firsts[0] if firsts else -1), (lasts[-1] if lasts else -1)


def percentile_finish(counts, percentages, lo, hi):
    """The percentile_approx finish (dataframe.py:1461-1529) of a host count grid with edges
    whose last axis is the percentile axis over [lo, hi]: the arithmetic of the device finish
    (vh_agg_percentile) in NumPy, for a count grid that did not stay in HBM.  The edge search of
    grid_find_edges (vaexfast.cpp:1574-1628) as a count: F = #{j : cum[j] < t},
    left = clip(F - 1, 0, N - 1), right = min(F, N - 1).  Shape (len(percentages),) + the
    central part of the outer axes; p = 0 / 100 give lo / hi in every cell."""
    counts = np.asarray(counts)
    central = counts[(slice(2, -1),) * (counts.ndim - 1) + (slice(1, None),)].astype(np.float64)
    cum = np.cumsum(central, -1)
    total = np.sum(central, -1)
    N = cum.shape[-1]
    lo, hi = np.float64(lo), np.float64(hi)
    out = np.empty((len(percentages),) + cum.shape[:-1], np.float64)

    def x(t):
        F = np.sum(cum < t[..., None], -1)
        left, right = np.clip(F - 1, 0, N - 1), np.minimum(F, N - 1)
        cl = np.take_along_axis(cum, left[..., None], -1)[..., 0]
        cr = np.take_along_axis(cum, right[..., None], -1)[..., 0]
        u = (t - cl) / (cr - cl)
        xl = lo + (left - 0.5) * (hi - lo) / np.float64(N - 3)
        xr = lo + (right - 0.5) * (hi - lo) / np.float64(N - 3)
        return xl + (xr - xl) * u

    with np.errstate(divide="ignore", invalid="ignore"):
        for i, p in enumerate(percentages):
            if p == 0 or p == 100:
                out[i] = lo if p == 0 else hi
                continue
            v = np.array((total + 1) * p / 100.)
            v[total == 0] = 0
            f, g = np.floor(v), np.ceil(v)
            x1, x2 = x(f), x(g)
            out[i] = x1 + (x2 - x1) * (v - f)
    return out


def mutual_information_finish(counts):
    """The mutual_information finish (dataframe.py:663-688 + kld.py:13-21) of a host count grid
    with edges whose first two axes are x and y: the arithmetic of the device finish
    (vh_agg_mutual_information) in NumPy, for a count grid that did not stay in HBM.  Over the
    central part of every axis, per outer cell: the sum over a > 0 of p * log(p / q) with
    p = a / T and q = rx * cy / (T * T) (T * T: the closed form of the reference's Q.sum()); an
    empty cell gives 0.  Shape: the central part of the outer axes."""
    counts = np.asarray(counts)
    a = counts[(slice(2, -1),) * counts.ndim]
    T = a.sum(axis=(0, 1), dtype=np.int64).astype(np.float64)
    rx = a.sum(axis=1, dtype=np.int64, keepdims=True).astype(np.float64)
    cy = a.sum(axis=0, dtype=np.int64, keepdims=True).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = a.astype(np.float64) / T
        q = (rx * cy) / (T * T)
        terms = np.where(a > 0, p * np.log(p / q), 0.0)
    return np.asarray(terms.sum(axis=(0, 1)))


def cov_finish(values, N):
    """The finish of DataFrame.cov (dataframe.py:1251-1268) over an AggCov grid: ``values``
    has ``2N + 2N**2`` fields on its last axis, the result the shape ``outer + (N, N)``."""
    values = np.asarray(values)
    counts = values[..., :N]
    sums = values[..., N:2 * N]
    with np.errstate(divide="ignore", invalid="ignore"):
        means = sums / counts
    # matrix of means * means.T
    meansxy = means[..., None] * means[..., None, :]
    counts = values[..., 2 * N:2 * N + N ** 2]
    sums = values[..., 2 * N + N ** 2:]
    shape = counts.shape[:-1] + (N, N)
    counts = counts.reshape(shape)
    sums = sums.reshape(shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        moments2 = sums / counts
    with np.errstate(invalid="ignore"):  # inf - inf in a cell holding an infinite value
        return moments2 - meansxy


def lasso_bounds(vertx, verty):
    """(meanx, meany, radius) of a lasso as SelectionLasso.evaluate computes them
    (selections.py:182-185): the vertex mean and the largest vertex distance from it; NaN for
    an empty lasso (nothing is inside it)."""
    vertx, verty = np.asarray(vertx, dtype=np.float64), np.asarray(verty, dtype=np.float64)
    if len(vertx) == 0:
        return float("nan"), float("nan"), float("nan")
    meanx, meany = vertx.mean(), verty.mean()
    with np.errstate(all="ignore"):
        radius = np.sqrt((meanx - vertx) ** 2 + (meany - verty) ** 2).max()
    return float(meanx), float(meany), float(radius)


def pnpoly(x, y, vertx, verty, meanx, meany, radius):
    """vaexfast.pnpoly (vaexfast.cpp:1757-1775) for host columns: the boolean mask of the points
    (x[k], y[k]) inside the polygon, the C loop's float64 arithmetic operation for operation.
    The loop runs over the edges, vectorised over the rows inside the radius, of which each
    edge touches only those whose y it straddles; row ranges are split over the host threads."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    vertx, verty = np.asarray(vertx, dtype=np.float64), np.asarray(verty, dtype=np.float64)
    meanx, meany, r2 = np.float64(meanx), np.float64(meany), np.float64(radius) * np.float64(radius)
    nvert = len(vertx)
    out = np.zeros(len(x), dtype=bool)

    def part(i0, i1):
        with np.errstate(all="ignore"):
            tx, ty = x[i0:i1], y[i0:i1]
            rows = np.flatnonzero((tx - meanx) * (tx - meanx) + (ty - meany) * (ty - meany) < r2)
            tx, ty = tx[rows], ty[rows]
            c = np.zeros(len(rows), dtype=bool)
            for i in range(nvert):
                j = i - 1 if i else nvert - 1
                k = np.flatnonzero((verty[i] > ty) != (verty[j] > ty))
                if len(k):
                    c[k] ^= tx[k] < (vertx[j] - vertx[i]) * (ty[k] - verty[i]) / (verty[j] - verty[i]) + vertx[i]
            out[i0:i1][rows] = c

    _run(part, len(x), min_split=1 << 16)
    return out
