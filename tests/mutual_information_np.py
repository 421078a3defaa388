"""NumPy restatement of the reference's mutual_information finish
(``packages/vaex-core/vaex/dataframe.py:663-688``, ``vaex/kld.py:13-21``,
``vaex/utils.py:119-142``), the yardstick of the device finish (``vh_agg_mutual_information``).

Input: a count grid WITH edges (every axis has slots 0 = NaN, 1 = underflow, 2..n+1 = bins,
n+2 = overflow) whose FIRST two axes are x and y and whose other axes are the binby axes.  The
reference counts without edges, so per outer central cell ``c`` it sees
``counts[2:-1, 2:-1, c]``; that slab goes through its arithmetic, operation for operation:
``np.nansum`` marginals, their outer product, ``P / P.sum()``, ``Q / Q.sum()``, the mask and
``np.sum``.

The tolerance per cell, with n the number of non-zero entries and t_k the cell's float64 terms:

    tol = (n + 64) * 2**-52 * (1 + sum |t_k|)

``n u sum|t|`` covers any summation order against any other, a few u per term cover the
division, the log (each side's within about 1 ulp) and the product, and the constant covers the
rounding of ``Q.sum()`` against the closed form ``T * T`` when the marginal products exceed 2^53.
"""
import numpy as np


def marginal_product(slab):
    """The product of the slab's two marginal distributions (what utils.py:127-142 builds for a
    2-d array through utils.py:119-124): NaN-ignoring sums over y and over x, multiplied as a
    column by a row."""
    over_y = np.nansum(slab, axis=1)
    over_x = np.nansum(slab, axis=0)
    return over_y[:, np.newaxis] * over_x[np.newaxis, :]


def mutual_information_terms(data):
    """kld.py:13-21 up to the final np.sum: the terms P[mask] * log(P[mask] / Q[mask])."""
    Q = marginal_product(data)
    P = data
    with np.errstate(divide="ignore", invalid="ignore"):  # an empty slab: 0 / 0, masked out below
        P = P / P.sum()
        Q = Q / Q.sum()
    mask = (P > 0) & (Q > 0)
    return P[mask] * np.log(P[mask] / Q[mask])


def mutual_information(data):
    return np.sum(mutual_information_terms(data))


def mutual_information_from_counts(counts):
    """(values, tol), both of the outer central shape ``tuple(s - 3 for s in counts.shape[2:])``."""
    counts = np.asarray(counts)
    assert counts.ndim >= 2
    outer = tuple(s - 3 for s in counts.shape[2:])
    values, tol = np.zeros(outer, np.float64), np.zeros(outer, np.float64)
    for c in np.ndindex(*outer):
        slab = counts[(slice(2, -1), slice(2, -1)) + tuple(i + 2 for i in c)].astype(np.float64)
        terms = mutual_information_terms(slab)
        values[c] = np.sum(terms)
        tol[c] = (len(terms) + 64) * 2.0 ** -52 * (1 + np.sum(np.abs(terms)))
    return values, tol
