"""The NumPy restatement of the percentile_approx finish (tests/percentile_np.py) pinned against
the reference's own known answers, so the GPU tests are not compared with a wrong yardstick.
No GPU: the count grids are built with NumPy."""
import numpy as np
import pytest

import percentile_np
from vaex_amd import hostops


def count_grid_1d(x, lo, hi, P):
    """AggCount grid with edges of BinnerScalar(x, lo, hi, P) (superagg_binners.cpp:14-56):
    slot 0 NaN, 1 underflow, 2..P+1 the bins, P+2 overflow."""
    x = np.asarray(x, np.float64)
    grid = np.zeros(P + 3, np.int64)
    scaled = (x - lo) * (1.0 / (hi - lo))
    for v, s in zip(x, scaled):
        if v != v:
            grid[0] += 1
        elif s < 0:
            grid[1] += 1
        elif s >= 1:
            grid[P + 2] += 1
        else:
            grid[int(s * P) + 2] += 1
    return grid


def test_reference_known_medians():
    """tests/percentile_approx_test.py:30-39: percentile_shape 256 over [0, 200]."""
    below = percentile_np.percentile_from_counts(count_grid_1d([0, 0, 10, 100, 200], 0, 200, 256), [50.], 0, 200)
    assert below.shape == (1,)
    np.testing.assert_allclose(below[0], 9.80392157, rtol=0, atol=1e-8)
    assert below[0] < 10
    above = percentile_np.percentile_from_counts(count_grid_1d([0, 0, 90, 100, 200], 0, 200, 256), [50.], 0, 200)
    np.testing.assert_allclose(above[0], 90.58823529, rtol=0, atol=1e-8)
    assert above[0] > 90


def test_empty_cell_and_end_percentages():
    rng = np.random.default_rng(1)
    counts = rng.integers(0, 50, size=(7, 6, 19)).astype(np.int64)
    counts[3, 2, :] = 0          # an empty central cell ...
    counts[3, 2, 0] = 11         # ... whose NaN slot is not
    out = percentile_np.percentile_from_counts(counts, [0, 30, 50, 100], -1.5, 2.5)
    assert out.shape == (4, 4, 3)
    assert np.isnan(out[1, 1, 0]) and np.isnan(out[2, 1, 0])
    np.testing.assert_array_equal(out[0], np.full((4, 3), -1.5))
    np.testing.assert_array_equal(out[3], np.full((4, 3), 2.5))
    assert np.isfinite(np.delete(out[2].ravel(), 1 * 3 + 0)).all()


def test_non_decreasing_in_percentage():
    """Between 0 and 100 the result interpolates a non-decreasing piecewise-linear x(t), so it is
    non-decreasing in p wherever finite.  The two ends are not part of that curve: p = 0 and
    p = 100 are pinned to lo and hi, while the reference's bin positions
    lo + (edge - 0.5) * (hi - lo) / (N - 3) reach below lo at edge 0 and above hi from edge
    P onwards (with mass in the overflow slot p = 99 gives 1.034 over [0, 1] here)."""
    rng = np.random.default_rng(2)
    counts = rng.integers(0, 30, size=(8, 35)).astype(np.int64)
    pcts = [0.1, 1, 5, 25, 50, 75, 95, 99, 99.9]
    out = percentile_np.percentile_from_counts(counts, pcts, 0., 1.)
    for cell in range(out.shape[1]):
        v = out[:, cell]
        v = v[np.isfinite(v)]
        assert len(v) >= 5
        assert (np.diff(v) >= 0).all(), v


@pytest.mark.parametrize("shape", [(40,), (9, 21), (6, 5, 12)])
def test_host_finish_equals_restatement(shape):
    """hostops.percentile_finish (the finish of a count grid that did not stay in HBM) uses the
    count form of the edge search: bit-identical to the literal loops."""
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 4, size=shape).astype(np.int64)
    counts[..., 5] = 0
    pcts = [0, 0.5, 25, 50, 75, 99.9, 100]
    np.testing.assert_array_equal(hostops.percentile_finish(counts, pcts, -3., 7.),
                                  percentile_np.percentile_from_counts(counts, pcts, -3., 7.))
