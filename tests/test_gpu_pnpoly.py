"""vh_pnpoly / vh_mask_combine (csrc/select.hip) through superutils.pnpoly / mask_combine:
device masks compared with the NumPy restatement (tests/pnpoly_np.py) byte for byte.  Points on
an integer lattice against integer-vertex polygons put many rows exactly on edges, on vertices
and at vertex heights, where ``>`` and ``<`` decide; the polygon's own vertices are test points
too (their distance from the mean reaches the radius).  Row counts around the wave (64), the
workgroup tile (PNPOLY_WG_ROWS) and past one grid step; vertex counts around the LDS chunk
(PNPOLY_LDS_EDGES), where the crossing parity is carried from chunk to chunk."""
import numpy as np
import pytest

from pnpoly_np import MODES, combine, pnpoly_np

pytestmark = pytest.mark.gpu

STAR = ([0, 2, 8, 3, 5, 0, -5, -3, -8, -2], [9, 3, 3, -1, -8, -3, -8, -1, 3, 3])  # concave
BOWTIE = ([-6, 6, -6, 6], [-6, 6, 6, -6])  # self-crossing
RECT_CLOSED = ([-3, 5, 5, -3, -3], [-2, -2, 6, 6, -2])  # horizontal / vertical edges, first vertex repeated
SHAPES = {"star": STAR, "bowtie": BOWTIE, "rect_closed": RECT_CLOSED}


def su():
    from vaex_amd import superutils
    return superutils


def dev(a):
    from vaex_amd.device import DeviceArray
    return DeviceArray.from_numpy(a)


def lattice(seed, n, span=10, poly=None):
    """n points: integer lattice points, free points, then the polygon's vertices, NaN / inf."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-span, span + 1, n).astype(np.float64)
    y = rng.integers(-span, span + 1, n).astype(np.float64)
    free = rng.random(n) < 0.3
    x[free] += rng.uniform(-0.5, 0.5, int(free.sum()))
    y[free] += rng.uniform(-0.5, 0.5, int(free.sum()))
    if poly is not None and n:
        k = min(n, len(poly[0]))
        x[:k], y[:k] = np.asarray(poly[0], np.float64)[:k], np.asarray(poly[1], np.float64)[:k]
    if n > 40:
        x[20::97], y[21::101] = np.nan, np.nan
        x[22::103], y[23::107], x[24::109], y[25::113] = np.inf, np.inf, -np.inf, -np.inf
    return x, y


def polygon(nvert, seed=0, span=10):
    """A star-shaped polygon of nvert integer vertices around the origin (rounding makes
    repeated vertices and horizontal / vertical edges once nvert passes the lattice's size)."""
    rng = np.random.default_rng(1000 + seed + nvert)
    angle = np.sort(rng.uniform(0, 2 * np.pi, nvert))
    radius = rng.uniform(0.3 * span, span, nvert)
    return np.round(radius * np.cos(angle)), np.round(radius * np.sin(angle))


def check(x, y, poly, prev=None, mode="replace", want=None):
    got = su().pnpoly(dev(x), dev(y), poly[0], poly[1], prev=None if prev is None else dev(prev), mode=mode)
    assert got.dtype == np.bool_ and len(got) == len(x)
    if want is None:
        want = pnpoly_np(x, y, *poly)
    np.testing.assert_array_equal(got.to_numpy().view(np.uint8), combine(prev, want, mode).view(np.uint8))
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, "tile-1", "tile", "tile+1", 1_000_003])
def test_row_counts(n):
    tile = su().PNPOLY_WG_ROWS
    assert tile == 2048
    n = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}.get(n, n)
    x, y = lattice(n, n, poly=STAR)
    want = check(x, y, STAR)
    if n >= 63:
        assert want.any() and not want.all()


@pytest.mark.parametrize("nvert", [0, 1, 2, 3, 4, "C-1", "C", "C+1", "3C+5"])
def test_vertex_counts(nvert):
    C = su().PNPOLY_LDS_EDGES
    assert C == 512
    nvert = {"C-1": C - 1, "C": C, "C+1": C + 1, "3C+5": 3 * C + 5}.get(nvert, nvert)
    poly = polygon(nvert)
    x, y = lattice(nvert, 3 * su().PNPOLY_WG_ROWS + 3, poly=poly)
    want = check(x, y, poly)
    assert want.any() == (nvert >= 3)
    prev = (np.arange(len(x)) % 3).astype(np.uint8)
    check(x, y, poly, prev=prev, mode="xor", want=want)


def test_many_rows_many_edges():
    """More than one LDS chunk under a grid of many workgroups."""
    poly = polygon(su().PNPOLY_LDS_EDGES + 1, seed=5, span=1000)
    x, y = lattice(3, 100_003, span=1000, poly=poly)
    want = check(x, y, poly)
    assert 0.2 < want.mean() < 0.8


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shapes_modes_and_prev(shape):
    poly = SHAPES[shape]
    x, y = lattice(len(shape), 5000, poly=poly)
    want = check(x, y, poly)
    assert want.any() and not want.all()
    prev = (np.random.default_rng(2).integers(0, 3, len(x))).astype(np.uint8)  # 2: not selected
    for mode in MODES:
        check(x, y, poly, prev=prev, mode=mode, want=want)
        check(x, y, poly, mode=mode, want=want)
    # prev as a bool mask, and in place of a host array
    got = su().pnpoly(dev(x), dev(y), *poly, prev=prev == 1, mode="subtract")
    np.testing.assert_array_equal(got.to_numpy(), (prev == 1) & ~want)


@pytest.mark.parametrize("dtx,dty", [("float32", "float64"), ("float64", "float32"), ("float32", "float32")])
def test_mixed_dtypes(dtx, dty):
    x, y = lattice(11, 4099, poly=STAR)
    x, y = (x + 0.1).astype(dtx), (y - 0.1).astype(dty)  # 0.1 rounds differently in float32
    check(x, y, STAR)
    with pytest.raises(TypeError):
        su().pnpoly(dev(np.zeros(len(x), np.int32)), dev(y), *STAR)


def test_unaligned_slices():
    """Columns, prev and out that do not start on a wide-load boundary take the per-row loads."""
    x, y = lattice(12, 6000, poly=BOWTIE)
    prev = (np.arange(6000) % 2).astype(np.uint8)
    dx, dy, dp = dev(x), dev(y), dev(prev)
    for off in (1, 3, 8):
        got = su().pnpoly(dx[off:], dy[off:], *BOWTIE, prev=dp[off:], mode="and")
        np.testing.assert_array_equal(got.to_numpy(), combine(prev[off:], pnpoly_np(x[off:], y[off:], *BOWTIE), "and"))


def test_mixed_host_device_and_errors():
    x, y = lattice(13, 1000, poly=STAR)
    np.testing.assert_array_equal(su().pnpoly(dev(x), y, *STAR).to_numpy(), pnpoly_np(x, y, *STAR))
    with pytest.raises(ValueError):
        su().pnpoly(dev(x), dev(y[:10]), *STAR)
    with pytest.raises(ValueError):
        su().pnpoly(dev(x), dev(y), *STAR, mode="nand")
    with pytest.raises(ValueError):
        su().pnpoly(dev(x), dev(y), [0, 1, 2], [0, 1])


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 2048 * 8 + 5, 1_000_003])
def test_mask_combine(n):
    rng = np.random.default_rng(n)
    a, b = rng.integers(0, 3, n).astype(np.uint8), rng.integers(0, 3, n).astype(np.uint8)  # 2: not selected
    da, db = dev(a), dev(b)
    for mode in MODES:
        got = su().mask_combine(da, db, mode)
        assert got.dtype == np.bool_
        np.testing.assert_array_equal(got.to_numpy().view(np.uint8), combine(a, b == 1, mode).view(np.uint8))
    np.testing.assert_array_equal(su().mask_combine(da).to_numpy().view(np.uint8), (a != 1).view(np.uint8))
    if n > 9:
        np.testing.assert_array_equal(su().mask_combine(da[3:], db[3:], "xor").to_numpy(), (a[3:] == 1) ^ (b[3:] == 1))
        np.testing.assert_array_equal(su().mask_combine(da[5:]).to_numpy(), a[5:] != 1)
