"""pnpoly_np (the NumPy restatement the GPU lasso is compared with) pinned three ways: against
the literal scalar transcription of the C loop, against the known answers of the reference's
test_lasso (tests/selection_test.py:181-197) and against that test's masked case; the host
path (hostops.pnpoly behind superutils.pnpoly) against it on the same points."""
import numpy as np
import pytest

from pnpoly_np import MODES, combine, pnpoly_np, pnpoly_scalar

STAR = ([0, 2, 8, 3, 5, 0, -5, -3, -8, -2], [9, 3, 3, -1, -8, -3, -8, -1, 3, 3])  # concave
BOWTIE = ([-4, 4, -4, 4], [-4, 4, 4, -4])  # self-crossing
RECT_CLOSED = ([-3, 5, 5, -3, -3], [-2, -2, 6, 6, -2])  # horizontal / vertical edges, first vertex repeated


def _points(seed, n=300):
    rng = np.random.default_rng(seed)
    lattice = rng.integers(-10, 11, (2, n // 2)).astype(np.float64)  # on edges, vertices, vertex heights
    free = rng.uniform(-10, 10, (2, n - n // 2))
    x, y = np.concatenate([lattice[0], free[0]]), np.concatenate([lattice[1], free[1]])
    x[::37] = np.nan
    y[5::41] = np.inf
    return x, y


@pytest.mark.parametrize("poly", [STAR, BOWTIE, RECT_CLOSED, ([], []), ([1], [1]), ([0, 3], [0, 3]),
                                  ([0.5, 7.25, -3.125], [-1.5, 2.75, 6.0])])
def test_matches_scalar_transcription(poly):
    x, y = _points(len(poly[0]))
    x, y = np.concatenate([x, poly[0]]), np.concatenate([y, poly[1]])  # the vertices themselves too
    want = pnpoly_scalar(x, y, *poly)
    np.testing.assert_array_equal(pnpoly_np(x, y, *poly), want)
    if len(poly[0]) >= 3:
        assert want.any() and not want.all()


def test_reference_known_answers():
    x = np.arange(10.0)
    y = x ** 2
    m = pnpoly_np(x, y, [-0.1, 5.1, 5.1, -0.1], [-0.1, -0.1, 4.1, 4.1])
    assert x[m].sum() == 0 + 1 + 2 and y[m].sum() == 0 + 1 + 4
    # the masked case: m ~= x with row 9 masked; the lasso holds rows 8 and 9, so 8 is left
    masked = np.ma.array(x, mask=x == 9)
    m = pnpoly_np(masked.data, y, [8 - 0.1, 9 + 0.1, 9 + 0.1, 8 - 0.1], [-0.1, -0.1, 1000, 1000])
    assert m.tolist() == [False] * 8 + [True, True]
    m = m & ~np.ma.getmaskarray(masked)
    assert x[m].sum() == 8 and y[m].sum() == 8 ** 2


@pytest.mark.parametrize("poly", [STAR, BOWTIE, RECT_CLOSED, ([], [])])
def test_host_path_matches(poly):
    from vaex_amd import hostops, superutils
    x, y = _points(7, 400)
    want = pnpoly_np(x, y, *poly)
    np.testing.assert_array_equal(superutils.pnpoly(x, y, *poly), want)
    np.testing.assert_array_equal(superutils.pnpoly(x.astype(np.float32), y, *poly), pnpoly_np(x.astype(np.float32), y, *poly))
    prev = (np.arange(len(x)) % 3).astype(np.uint8)  # bytes of 2 are not selected
    for mode in MODES:
        np.testing.assert_array_equal(superutils.pnpoly(x, y, *poly, prev=prev, mode=mode), combine(prev, want, mode))
        np.testing.assert_array_equal(superutils.pnpoly(x, y, *poly, mode=mode), combine(None, want, mode))
    # the threaded split gives the same mask
    big = np.tile(x, 700), np.tile(y, 700)
    np.testing.assert_array_equal(hostops.pnpoly(*big, *poly, *hostops.lasso_bounds(*poly)), np.tile(want, 700))
