"""NumPy restatement of the lasso's point-in-polygon test: ``vaexfast.pnpoly``
(vaexfast.cpp:1757-1775) with the mean / radius that ``SelectionLasso.evaluate``
(selections.py:182-185) hands it, and the mode table ``_select_functions``
(selections.py:11-36).  Plain float64 numpy, one operation per C operation, every edge against
every row: the GPU kernel and the host path are compared with it byte for byte.
``pnpoly_scalar`` is the literal scalar transcription of the C loop that pins it."""
import numpy as np

MODES = ["replace", "and", "or", "xor", "subtract"]


def lasso_bounds(vertx, verty):
    vertx, verty = np.asarray(vertx, dtype=np.float64), np.asarray(verty, dtype=np.float64)
    if len(vertx) == 0:  # the reference cannot take an empty lasso; here nothing is inside it
        return np.float64("nan"), np.float64("nan"), np.float64("nan")
    meanx, meany = vertx.mean(), verty.mean()
    with np.errstate(all="ignore"):
        radius = np.sqrt((meanx - vertx) ** 2 + (meany - verty) ** 2).max()
    return meanx, meany, radius


def pnpoly_np(x, y, vertx, verty):
    """bool mask of the points inside; x / y of any float dtype are read as float64."""
    tx, ty = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    vx, vy = np.asarray(vertx, dtype=np.float64), np.asarray(verty, dtype=np.float64)
    meanx, meany, radius = lasso_bounds(vx, vy)
    c = np.zeros(len(tx), dtype=bool)
    with np.errstate(all="ignore"):
        d = (tx - meanx) * (tx - meanx) + (ty - meany) * (ty - meany)
        for i in range(len(vx)):
            j = i - 1 if i else len(vx) - 1
            straddle = (vy[i] > ty) != (vy[j] > ty)
            q = (vx[j] - vx[i]) * (ty - vy[i]) / (vy[j] - vy[i]) + vx[i]
            c ^= straddle & (tx < q)
        return c & (d < radius * radius)


def pnpoly_scalar(x, y, vertx, verty):
    """The C loop, statement for statement, on Python floats (IEEE float64)."""
    vx, vy = [float(v) for v in vertx], [float(v) for v in verty]
    nvert = len(vx)
    meanx, meany, radius = [float(v) for v in lasso_bounds(vx, vy)]
    radius_squared = radius * radius
    mask = np.zeros(len(x), dtype=bool)
    for k in range(len(x)):
        testx, testy = float(x[k]), float(y[k])
        c = False
        distancesq = (testx - meanx) * (testx - meanx) + (testy - meany) * (testy - meany)
        if distancesq < radius_squared:
            j = nvert - 1
            for i in range(nvert):
                if ((vy[i] > testy) != (vy[j] > testy)) and \
                        (testx < (vx[j] - vx[i]) * (testy - vy[i]) / (vy[j] - vy[i]) + vx[i]):
                    c = not c
                j = i
            mask[k] = c
    return mask


def combine(prev, new, mode):
    """_select_functions; prev None: no previous selection.  prev bytes: only 1 is selected."""
    new = np.asarray(new, dtype=bool)
    if prev is None:
        return ~new if mode == "subtract" else new
    prev = np.asarray(prev).view(np.uint8) == 1 if np.asarray(prev).dtype == np.bool_ else np.asarray(prev) == 1
    return {"replace": new, "and": prev & new, "or": prev | new, "xor": prev ^ new, "subtract": prev & ~new}[mode]
