"""The AggCov yardstick (tests/cov_np.py) against the reference's own definitions: the
bincount form equals the literal loops bit for bit, the finishes equal ``np.cov(bias=1)``, and
the reference's known answers (``tests/agg_test.py:54-99``, 10-row frame ``x = arange(10)``,
``y = x**2``) come out of it.  No GPU."""
import numpy as np
import pytest

import cov_np
from oracle import oracle


def _columns(N, n=300, seed=3):
    rng = np.random.default_rng(seed)
    cols = [rng.normal(size=n) * 10 for _ in range(N)]
    cols[0][rng.random(n) < 0.1] = np.nan            # NaN in x only
    if N > 1:
        cols[1][rng.random(n) < 0.1] = np.nan        # in y only, and in both by chance ...
        cols[0][5] = cols[1][5] = np.nan             # ... and in both for sure
        cols[0][7], cols[1][7] = np.inf, 0.0         # inf * 0
    cols[0][11] = np.inf
    return cols


@pytest.mark.parametrize("N", [1, 2, 3])
def test_bincount_form_equals_the_loops(N):
    cols = _columns(N)
    n = len(cols[0])
    key = np.random.default_rng(9).uniform(-0.2, 1.2, n)
    key[::29] = np.nan
    b = oracle.Binner("scalar", key, vmin=0.0, vmax=1.0, bins=4)  # 7 cells
    idx = oracle.bin_indices([b], n)
    assert b.shape() == 7
    keep = np.random.default_rng(10).random(n) < 0.7
    for k in (None, keep):
        a = cov_np.op_cov(idx, 7, cols, k)
        want = cov_np.op_cov_loop(idx, 7, cols, k)
        np.testing.assert_array_equal(a, want)
    # the data did reach every cell, the inf and (with a second column) the inf * 0 row
    whole = cov_np.op_cov(idx, 7, cols)
    assert len(np.unique(idx)) == 7 and np.isinf(whole).any() and (N == 1 or np.isnan(whole).any())


@pytest.mark.parametrize("N", [2, 3])
def test_finish_matches_numpy_cov(N):
    rng = np.random.default_rng(N)
    cols = [rng.normal(size=300) for _ in range(N)]
    cols[1] = cols[1] + 0.5 * cols[0]
    values = cov_np.op_cov(np.zeros(300, np.uint64), 1, cols)[0]
    cov = cov_np.cov_finish(values, N)
    want = np.cov(cols, bias=1)
    np.testing.assert_array_almost_equal(cov, want)
    np.testing.assert_array_almost_equal(cov_np.correlation_finish(cov), want[0, 1] / (want[0, 0] * want[1, 1]) ** 0.5)


def _np_correlation(x, y):
    c = np.cov([x, y], bias=1)
    return c[0, 1] / (c[0, 0] * c[1, 1]) ** 0.5


def _kat(xc, yc, by=None, limits=None, shape=None, keep=None):
    n = len(xc)
    if by is None:
        values = cov_np.op_cov(np.zeros(n, np.uint64), 1, [xc, yc], keep)[0]
    else:
        b = oracle.Binner("scalar", by, vmin=limits[0], vmax=limits[1], bins=shape)
        values = cov_np.op_cov(oracle.bin_indices([b], n), shape + 3, [xc, yc], keep)[2:-1]
    return cov_np.correlation_finish(cov_np.cov_finish(values, 2))


def test_reference_known_answers():
    x = np.arange(10, dtype=np.float64)
    y = x ** 2
    sel = x < 5
    np.testing.assert_array_almost_equal(_kat(y, y), 1.0)
    np.testing.assert_array_almost_equal(_kat(y, -y), -1.0)
    np.testing.assert_array_almost_equal(_kat(x, y), _np_correlation(x, y))
    np.testing.assert_array_almost_equal(_kat(x, y, keep=sel), _np_correlation(x[:5], y[:5]))
    np.testing.assert_array_almost_equal(_kat(x, y, x, [0, 10], 1), [_np_correlation(x, y)])
    np.testing.assert_array_almost_equal(_kat(x, y, y, [0, 9 ** 2 + 1], 1, sel), [_np_correlation(x[:5], y[:5])])
    i = 5
    np.testing.assert_array_almost_equal(_kat(x, y, x, [0, 10], 2),
                                         [_np_correlation(x[:i], y[:i]), _np_correlation(x[i:], y[i:])])
    np.testing.assert_array_almost_equal(_kat(x, y, x, [0, 10], 2, sel), [_np_correlation(x[:i], y[:i]), np.nan])
    i = 7
    np.testing.assert_array_almost_equal(_kat(x, y, y, [0, 9 ** 2 + 1], 2),
                                         [_np_correlation(x[:i], y[:i]), _np_correlation(x[i:], y[i:])])
    np.testing.assert_array_almost_equal(_kat(x, y, y, [0, 9 ** 2 + 1], 2, sel), [_np_correlation(x[:5], y[:5]), np.nan])


def test_grid_view_is_fortran_over_the_binners():
    flat = np.arange(3 * 4 * 6, dtype=np.float64).reshape(12, 6)  # shapes (3, 4), F = 6
    v = cov_np.grid_view(flat, (3, 4))
    assert v.shape == (3, 4, 6)
    assert v[2, 1, 5] == flat[2 + 1 * 3, 5]


def test_hostops_finish_is_the_reference_expression():
    """vaex_amd.hostops.cov_finish is plain NumPy: checked here without a GPU when the package
    imports (its HIP library is only loaded on first use)."""
    from vaex_amd import hostops
    cols = _columns(3)
    values = cov_np.op_cov(np.arange(300, dtype=np.uint64) % 5, 5, cols)
    np.testing.assert_array_equal(hostops.cov_finish(values, 3), cov_np.cov_finish(values, 3))
