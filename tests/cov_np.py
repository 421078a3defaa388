"""NumPy restatement of the reference's OP_COV statistic (``op_cov``,
``packages/vaex-core/src/vaexfast.cpp:1070-1104``) and of the finishes of ``DataFrame.cov`` /
``correlation`` (``vaex/dataframe.py:1251-1268,1141-1144``): the yardstick of ``AggCov``.

Per cell ``F = 2N + 2N**2`` float64 fields: ``[0, N)`` counts of non-NaN values, ``[N, 2N)``
their sums, ``[2N, 2N + N*N)`` at ``r + c * N`` the rows where columns c and r are both
non-NaN, ``[2N + N*N, F)`` at ``r + c * N`` the sum of ``v_c * v_r`` over those rows.  A row's
cell is ``idx[row]`` (``oracle.bin_indices``, this project's binners); ``keep`` is the data mask
(1 = the row contributes).
"""
import numpy as np


def fields(N):
    return 2 * N + 2 * N * N


def op_cov_loop(idx, L, columns, keep=None):
    """The reference's literal nested loops, row by row, into an (L, F) float64 array."""
    N = len(columns)
    Nsquare = N * N
    out = np.zeros((L, fields(N)), np.float64)
    columns = [np.asarray(c, np.float64) for c in columns]
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(idx)):
            if keep is not None and not keep[i]:
                continue
            outputs = out[int(idx[i])]
            for col in range(N):
                value = columns[col][i]
                if not np.isnan(value):
                    outputs[col] += 1
                    outputs[col + N] += value
                    # diagonal elements
                    outputs[N * 2 + col + col * N] += 1
                    outputs[N * 2 + Nsquare + col + col * N] += value * value
                    value_x = value
                    # off diagonal
                    for row in range(col + 1, N):
                        value_y = columns[row][i]
                        if not np.isnan(value_y):
                            index_1d_a = row + col * N
                            index_1d_b = col + row * N
                            outputs[N * 2 + index_1d_a] += 1
                            outputs[N * 2 + index_1d_b] = outputs[N * 2 + index_1d_a]
                            outputs[N * 2 + Nsquare + index_1d_a] += value_x * value_y
                            outputs[N * 2 + Nsquare + index_1d_b] = outputs[N * 2 + Nsquare + index_1d_a]
    return out


def op_cov(idx, L, columns, keep=None):
    """The same fields with one ``np.bincount`` per field (it accumulates in row order, like
    the reference's loop)."""
    N = len(columns)
    idx = np.asarray(idx).astype(np.int64)
    columns = [np.asarray(c, np.float64) for c in columns]
    keep = np.ones(len(idx), bool) if keep is None else np.asarray(keep).astype(bool)
    out = np.zeros((L, fields(N)), np.float64)
    ok = [keep & ~np.isnan(c) for c in columns]

    def binned(sel, weights=None):
        w = None if weights is None else weights[sel]
        return np.bincount(idx[sel], weights=w, minlength=L).astype(np.float64)

    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(N):
            out[:, c] = binned(ok[c])
            out[:, N + c] = binned(ok[c], columns[c])
            for r in range(c, N):
                both = ok[c] & ok[r]
                cnt = binned(both)
                s = binned(both, columns[c] * columns[r])
                for a, b in ((r, c), (c, r)):
                    out[:, 2 * N + a + b * N] = cnt
                    out[:, 2 * N + N * N + a + b * N] = s
    return out


def cov_finish(values, N):
    """dataframe.py:1251-1268."""
    counts = values[..., :N]
    sums = values[..., N:2 * N]
    with np.errstate(divide='ignore', invalid='ignore'):
        means = sums / counts
    # matrix of means * means.T
    meansxy = means[..., None] * means[..., None, :]

    counts = values[..., 2 * N:2 * N + N**2]
    sums = values[..., 2 * N + N**2:]
    shape = counts.shape[:-1] + (N, N)
    counts = counts.reshape(shape)
    sums = sums.reshape(shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        moments2 = sums / counts
    with np.errstate(invalid='ignore'):  # inf - inf in a cell holding an infinite value
        cov_matrix = moments2 - meansxy
    return cov_matrix


def correlation_finish(cov):
    """dataframe.py:1141-1144."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return cov[..., 0, 1] / (cov[..., 0, 0] * cov[..., 1, 1])**0.5


def grid_view(flat, shape):
    """An (L, F) array as ``shape + (F,)``: the binner axes in Fortran order (the first binner
    fastest), the field axis last -- what ``np.asarray(AggCov)`` presents."""
    F = flat.shape[-1]
    return flat.reshape(tuple(shape)[::-1] + (F,)).transpose(tuple(range(len(shape) - 1, -1, -1)) + (len(shape),))
