"""``DataFrame.sort`` / ``extract`` -- the reference's row reordering
(``packages/vaex-core/vaex/dataframe.py:4216-4233,4420-4461``): ``sort`` is ``argsort`` /
``lexsort`` of the key expressions followed by ``take``, ``extract`` is the kept rows of a
filtered frame (so ``df.extract().take(indices)`` takes from the kept rows; ``take`` itself still
refuses indices that address a filtered frame's kept rows, join.py).  On a frame with HBM
columns both stay on the device: the kept rows are
``superutils.mask_rows`` of the filter's device mask, the order is ``superutils.argsort_device``
of the key columns over those rows, and the columns are gathered by ``vh_take`` (``join.gather``;
host columns of a mixed frame are gathered on the host threads).  A frame with no HBM column
uses NumPy for the same order."""
import numpy as np

from .device import DeviceArray, DeviceMaskedArray
from .join import _chunks, _host_indices, take_rows
from .strings import DeviceStringArray, encode, rank_codes
from .superutils import argsort_device, mask_rows, take_device


def _rows(df):
    """The row count of a frame whose executor owns every row (a multi-rank executor owns a
    shard: reordering one shard would be wrong; raises NotImplementedError as join does)."""
    _chunks(df)
    return df.length_unfiltered()


def kept_rows(df):
    """The unfiltered row numbers a filtered frame keeps, ascending: a DeviceArray
    (``mask_rows`` of the filter's device mask) on a frame with HBM columns, else a host array."""
    n = _rows(df)
    if df.is_device_resident():
        return mask_rows(df.device_keep_mask(0, n))
    return np.flatnonzero(df.evaluate_filter_mask(0, n))


def compact_device(column, mask):
    """``column[mask != 0]`` for a DeviceArray (or DeviceMaskedArray: data and mask) column and a
    device byte mask, in HBM."""
    if isinstance(column, DeviceMaskedArray):
        return DeviceMaskedArray(*take_device([column.data, column.mask], mask_rows(mask)))
    return take_device([column], mask_rows(mask))[0]


def _host_key(key):
    key = key.to_numpy() if isinstance(key, DeviceArray) else np.ma.getdata(key)
    return key.view(np.int64) if key.dtype.kind in "mM" else key


def _host_order(keys, rows, ascending, single):
    keys = [_host_key(k) for k in keys]
    if rows is not None:
        rows = _host_indices(rows)
        keys = [k[rows] for k in keys]
    order = np.argsort(keys[0], kind="stable") if single else np.lexsort(keys[::-1])
    if not ascending:
        order = order[::-1]
    return order if rows is None else rows[order]


def _string_ranks(column):
    """A string key as an int32 column that sorts like it: the rank of each row's string among
    the column's distinct strings (the encoder's codes remapped, strings.rank_codes)."""
    codes, sset = encode(column)
    return rank_codes(codes, sset.key_array())[0]


def argsort(df, by, ascending=True):
    """The unfiltered row numbers of the rows ``df`` keeps, in the order of ``by`` (an
    expression, or a list / tuple of them with the first the most significant): stable, NaN
    last; descending is the exact reverse.  A DeviceArray when the frame has HBM columns."""
    single = not isinstance(by, (list, tuple))
    bys = [str(by)] if single else [str(b) for b in by]
    if not bys:
        raise ValueError("sort needs at least one key")
    n = _rows(df)
    keys = [df._eval_host(b, 0, n) for b in bys]
    for b, k in zip(bys, keys):
        if isinstance(k, DeviceMaskedArray):
            raise NotImplementedError(f"sort by the masked HBM column / expression {b!r} is not supported")
    keys = [_string_ranks(k) if isinstance(k, DeviceStringArray) else k for k in keys]
    rows = kept_rows(df) if df.filtered else None
    if not df.is_device_resident() or any(np.ma.isMaskedArray(k) for k in keys):
        return _host_order(keys, rows, ascending, single)
    # a host column of a mixed frame that is a key is staged; datetimes sort as int64
    dkeys = [k if isinstance(k, DeviceArray) else DeviceArray.from_numpy(_host_key(np.asarray(k))) for k in keys]
    return argsort_device(dkeys, rows=rows, ascending=ascending)


def sort(df, by, ascending=True, kind="quicksort"):
    """dataframe.py:4420-4461.  ``kind`` is accepted; the order is always the stable one
    (a valid answer for every NumPy kind).  The result holds the kept rows only and has no
    filter; virtual columns, variables, categories and selections carry over."""
    return take_rows(df, argsort(df, by, ascending), dropfilter=True)


def extract(df):
    """dataframe.py:4216-4233: a frame of the kept rows, the filter dropped (a copy when the
    frame has no filter)."""
    if not df.filtered:
        return df.copy()
    return take_rows(df, kept_rows(df), dropfilter=True)
