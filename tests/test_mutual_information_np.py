"""The NumPy restatement of the mutual_information finish (tests/mutual_information_np.py) and
hostops.mutual_information_finish (the finish of a count grid that did not stay in HBM) pinned
against each other, against closed forms and against the reference's known answer, so the GPU
tests are not compared with a wrong yardstick.  No GPU: the count grids are built with NumPy."""
import numpy as np
import pytest

import mutual_information_np as mi_np
from vaex_amd import hostops


def with_edges(central, rng=None):
    """A count grid with edges around ``central`` (x, y, outer...): zeros in the edge slots, or
    random junk, which the finish must ignore."""
    central = np.asarray(central, np.int64)
    shape = tuple(s + 3 for s in central.shape)
    grid = np.zeros(shape, np.int64) if rng is None else rng.integers(1, 50, size=shape).astype(np.int64)
    grid[(slice(2, -1),) * central.ndim] = central
    return grid


def count_grid_2d(x, y, xlim, ylim, shape):
    """AggCount grid with edges of two BinnerScalars (superagg_binners.cpp:14-56)."""
    grid = np.zeros((shape + 3, shape + 3), np.int64)

    def slot(v, lo, hi):
        s = (v - lo) * (1.0 / (hi - lo))
        return 0 if v != v else 1 if s < 0 else shape + 2 if s >= 1 else int(s * shape) + 2

    for a, b in zip(x, y):
        grid[slot(a, *xlim), slot(b, *ylim)] += 1
    return grid


def agree(counts):
    values, tol = mi_np.mutual_information_from_counts(counts)
    got = hostops.mutual_information_finish(counts)
    assert got.shape == values.shape and got.dtype == np.float64
    assert (np.abs(got - values) <= tol).all(), (got, values, tol)
    return got, values, tol


@pytest.mark.parametrize("outer", [(), (4,), (3, 2), (2, 3, 2), (2, 2, 2, 2)])
def test_hostops_matches_restatement(outer):
    rng = np.random.default_rng(len(outer))
    central = rng.integers(0, 30, size=(17, 9) + outer)
    central[rng.random(central.shape) < 0.3] = 0
    if outer:
        central[(slice(None), slice(None)) + (0,) * len(outer)] = 0  # an empty cell
    got, values, _ = agree(with_edges(central, rng))
    assert got.shape == outer
    if outer:
        assert got[(0,) * len(outer)] == 0.0 and values[(0,) * len(outer)] == 0.0  # exactly
        assert (got.ravel()[1:] > 0).all()


def test_large_counts():
    """Totals below 2^53, marginal products above it."""
    rng = np.random.default_rng(3)
    central = rng.integers(0, 4, size=(40, 33, 3)).astype(np.int64) << 40
    got, values, tol = agree(with_edges(central, rng))
    assert (tol < 1e-9).all() and (values > 0).all()


@pytest.mark.parametrize("M", [2, 7, 64])
def test_diagonal_gives_log_m(M):
    got, values, tol = agree(with_edges(np.eye(M, dtype=np.int64) * 5))
    assert abs(got - np.log(M)) <= tol and abs(values - np.log(M)) <= tol


def test_closed_forms_zero():
    rng = np.random.default_rng(5)
    one = np.zeros((8, 6), np.int64)
    one[3, 2] = 1000
    product = np.outer(rng.integers(1, 9, size=12), rng.integers(1, 9, size=7))
    for central in (one, rng.integers(1, 9, size=(1, 20)), rng.integers(1, 9, size=(20, 1)), product):
        got, values, tol = agree(with_edges(central, rng))
        assert abs(got) <= tol and abs(values) <= tol


def test_reference_known_answer():
    """tests/agg_test.py:442-447: x = arange(10.), y = x**2, mi_shape 32 over [[0, 9], [0, 81]];
    the rows x = 9 and y = 81 fall in the overflow slot."""
    x = np.arange(10.)
    counts = count_grid_2d(x, x ** 2, [0, 9], [0, 81], 32)
    assert counts[2:-1, 2:-1].sum() == 9 and counts[-1, -1] == 1
    got, values, tol = agree(counts)
    np.testing.assert_almost_equal(values, 2.043192, 6)
    np.testing.assert_almost_equal(got, 2.043192, 6)
    assert abs(values - 2.0431918705451206) <= tol
