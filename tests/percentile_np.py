"""NumPy restatement of the reference's percentile_approx finish
(``packages/vaex-core/vaex/dataframe.py:1461-1529`` with ``grid_find_edges``,
``src/vaexfast.cpp:1574-1628``), the yardstick of the device finish (``vh_agg_percentile``).

``counts`` is a count grid with edges (slot 0 NaN / missing, 1 underflow, 2..n+1 the bins,
n+2 overflow on every axis) whose LAST axis is the percentile axis over ``[lo, hi]``.  The
edge search is written with the reference's literal ``while`` loops (the bound tested before
``cum[left + 1]`` is read, and the same rule for a grid with no outer axes), not with the
count the kernel uses, so the comparison checks that closed form too.  Unlike the reference,
percentages 0 and 100 are broadcast to the outer shape.
"""
import numpy as np


def find_edges(cum, t):
    """grid_find_edges for one cell: ``cum`` a list of N cumulative counts."""
    n = len(cum)
    left = 0
    while left < n - 1 and cum[left + 1] < t:
        left += 1
    right = left
    while right < n - 1 and cum[right] < t:
        right += 1
    return left, right


def percentile_from_counts(counts, percentages, lo, hi):
    """Array of shape (len(percentages),) + central outer shape."""
    counts = np.asarray(counts).astype(np.float64)
    nonnans = (slice(2, -1),) * (counts.ndim - 1) + (slice(1, None),)
    cumulative_grid = np.cumsum(counts[nonnans], -1)
    totalcounts = np.sum(counts[nonnans], -1)
    outer = cumulative_grid.shape[:-1]
    N = cumulative_grid.shape[-1]
    lo, hi = np.float64(lo), np.float64(hi)
    out = np.empty((len(percentages),) + outer, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for cell in np.ndindex(*outer):
            cum = cumulative_grid[cell]
            cum_list = cum.tolist()
            total = totalcounts[cell]

            def calculate_x(t):
                left, right = find_edges(cum_list, float(t))
                u = (t - cum[left]) / (cum[right] - cum[left])
                xleft = lo + (left - 0.5) * (hi - lo) / (N - 3)
                xright = lo + (right - 0.5) * (hi - lo) / (N - 3)
                return xleft + (xright - xleft) * u

            for i, p in enumerate(percentages):
                if p == 0:
                    out[(i,) + cell] = lo
                    continue
                if p == 100:
                    out[(i,) + cell] = hi
                    continue
                value = (total + 1) * p / 100.
                if total == 0:
                    value = np.float64(0)
                floor_value, ceil_value = np.floor(value), np.ceil(value)
                x1 = calculate_x(floor_value)
                x2 = calculate_x(ceil_value)
                out[(i,) + cell] = x1 + (x2 - x1) * (value - floor_value)
    return out
