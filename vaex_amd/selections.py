"""The selection model (``packages/vaex-core/vaex/selections.py``): a selection is a chain of
nodes, each combining with the one before it by a mode (replace / and / or / xor / subtract).

A chain of :class:`SelectionExpression` / :class:`SelectionInvert` nodes folds into one
expression string (:meth:`Selection.fold`), which the frame evaluates like any selection
expression: one fused device program on an HBM frame, one numpy evaluation on a host frame.
Only a chain holding a :class:`SelectionLasso` (or, on a host frame, a
:class:`SelectionDropNa`) is evaluated node by node: on a host frame into numpy masks over the
filtered rows (``evaluate``), on an HBM frame into device masks over all rows of the chunk
(``evaluate_device``; the lasso runs ``vh_pnpoly`` with its previous mask fused in, and nothing
but the vertex arrays crosses the host link).
"""
import numpy as np

from .device import DeviceArray


def _select_replace(maskold, masknew):
    return masknew


def _select_and(maskold, masknew):
    return masknew if maskold is None else maskold & masknew


def _select_or(maskold, masknew):
    return masknew if maskold is None else maskold | masknew


def _select_xor(maskold, masknew):
    return masknew if maskold is None else maskold ^ masknew


def _select_subtract(maskold, masknew):
    return ~masknew if maskold is None else (maskold) & ~masknew


_select_functions = {"replace": _select_replace,
                     "and": _select_and,
                     "or": _select_or,
                     "xor": _select_xor,
                     "subtract": _select_subtract}

# the folded forms of mode(p, n)
_fold_formats = {"and": "({p}) & ({n})", "or": "({p}) | ({n})", "xor": "({p}) ^ ({n})", "subtract": "({p}) & ~({n})"}


def _check_mode(mode):
    if mode not in _select_functions:
        raise ValueError("unknown selection mode %r, expected one of %s" % (mode, ", ".join(_select_functions)))


def _freeze(value):
    """A hashable form of a ``to_dict()`` value (the key of a per-block mask cache entry)."""
    if isinstance(value, dict):
        return tuple((k, _freeze(v)) for k, v in sorted(value.items()))
    if isinstance(value, (list, tuple, np.ndarray)):
        return tuple(_freeze(v) for v in value)
    if isinstance(value, (float, np.floating)):
        return repr(float(value))  # NaN equals NaN, -0.0 differs from 0.0
    return value


def _make_list(sequence):
    return np.asarray(sequence).tolist()


def _device_not(mask):
    from .superutils import mask_combine
    return mask_combine(mask, None)


class Selection(object):
    expressions = []

    def __init__(self, previous_selection, mode):
        # we don't care about the previous selection if we simply replace the current selection
        self.previous_selection = previous_selection if mode != "replace" else None
        self.mode = mode

    def dependencies(self):
        """The expressions this selection and the ones before it are evaluated from."""
        own = [str(e) for e in self.expressions]
        return own + (self.previous_selection.dependencies() if self.previous_selection else [])

    def fold(self, df=None):
        """The chain as one expression string, or None when a node of it has none."""
        return None

    def _fold_mode(self, new, df):
        """``mode(previous, new)`` for the expression string ``new`` as one expression string."""
        if self.previous_selection is None:
            return "~(%s)" % new if self.mode == "subtract" else new
        previous = self.previous_selection.fold(df)
        if previous is None:
            return None
        return _fold_formats[self.mode].format(p=previous, n=new)

    def key(self):
        return _freeze(self.to_dict())

    def _previous_dict(self):
        return self.previous_selection.to_dict() if self.previous_selection else None

    def _previous_mask(self, df, i1, i2, filter_mask):
        if self.previous_selection is None:
            return None
        return self.previous_selection.evaluate(df, i1, i2, filter_mask)

    def evaluate(self, df, i1, i2, filter_mask=None):
        """Host frame: the boolean mask over the rows [i1, i2) that pass ``filter_mask``."""
        folded = self.fold(df)
        if folded is not None:
            return df._expression_mask(folded, i1, i2, filter_mask)
        return self._evaluate(df, i1, i2, filter_mask)

    def evaluate_device(self, df, i1, i2):
        """HBM frame: the device mask (0 / 1 bytes) over all rows [i1, i2); the filter is not
        applied (``DataFrame.device_keep_mask`` ands it in)."""
        folded = self.fold(df)
        if folded is not None:
            return df._eval_row_mask(folded, i1, i2)  # a missing value selects nothing
        return self._evaluate_device(df, i1, i2)

    def _own_expression(self, df):
        """This node's own mask as an expression string on ``df``, or None when it has none."""
        return None

    def _evaluate_device(self, df, i1, i2):
        """A node with an expression of its own behind a chain that does not fold."""
        from .superutils import mask_combine
        previous_mask = self.previous_selection.evaluate_device(df, i1, i2)
        current_mask = df._eval_row_mask(self._own_expression(df), i1, i2)
        return mask_combine(previous_mask, current_mask, self.mode)

    def __repr__(self):
        return "%s(%r)" % (type(self).__name__, self.to_dict())


class SelectionExpression(Selection):
    def __init__(self, boolean_expression, previous_selection, mode):
        _check_mode(mode)
        super(SelectionExpression, self).__init__(previous_selection, mode)
        self.boolean_expression = str(boolean_expression)
        self.expressions = [self.boolean_expression]

    def to_dict(self):
        return dict(type="expression", boolean_expression=str(self.boolean_expression), mode=self.mode,
                    previous_selection=self._previous_dict())

    def fold(self, df=None):
        return self._fold_mode(self.boolean_expression, df)

    def _own_expression(self, df):
        return self.boolean_expression

    def _evaluate(self, df, i1, i2, filter_mask):  # the chain before it holds a lasso or a drop-na
        previous_mask = self._previous_mask(df, i1, i2, filter_mask)
        current_mask = df._expression_mask(self.boolean_expression, i1, i2, filter_mask)
        return _select_functions[self.mode](previous_mask, current_mask)


class SelectionInvert(Selection):
    def __init__(self, previous_selection):
        if previous_selection is None:
            raise ValueError("there is no selection to invert")
        super(SelectionInvert, self).__init__(previous_selection, "")
        self.expressions = []

    def to_dict(self):
        return dict(type="invert", previous_selection=self._previous_dict())

    def fold(self, df=None):
        previous = self.previous_selection.fold(df)
        return None if previous is None else "~(%s)" % previous

    def _evaluate(self, df, i1, i2, filter_mask):
        return ~self._previous_mask(df, i1, i2, filter_mask)

    def _evaluate_device(self, df, i1, i2):
        return _device_not(self.previous_selection.evaluate_device(df, i1, i2))


class SelectionLasso(Selection):
    def __init__(self, boolean_expression_x, boolean_expression_y, xseq, yseq, previous_selection, mode):
        _check_mode(mode)
        super(SelectionLasso, self).__init__(previous_selection, mode)
        self.boolean_expression_x = str(boolean_expression_x)
        self.boolean_expression_y = str(boolean_expression_y)
        self.xseq = xseq
        self.yseq = yseq
        if len(xseq) != len(yseq):
            raise ValueError("xseq and yseq hold %d and %d vertices" % (len(xseq), len(yseq)))
        self.expressions = [self.boolean_expression_x, self.boolean_expression_y]

    def to_dict(self):
        return dict(type="lasso",
                    boolean_expression_x=str(self.boolean_expression_x),
                    boolean_expression_y=str(self.boolean_expression_y),
                    xseq=_make_list(self.xseq),
                    yseq=_make_list(self.yseq),
                    mode=self.mode,
                    previous_selection=self._previous_dict())

    def _evaluate(self, df, i1, i2, filter_mask):
        """selections.py:172-204: x / y are evaluated on the filtered rows, a row whose x or y
        is masked is never selected."""
        from .superutils import pnpoly
        previous_mask = self._previous_mask(df, i1, i2, filter_mask)
        blockx = df._eval_host(self.boolean_expression_x, i1, i2, filter_mask)
        blocky = df._eval_host(self.boolean_expression_y, i1, i2, filter_mask)
        excluding_mask = None
        for block in (blockx, blocky):
            if np.ma.isMaskedArray(block):
                m = np.ma.getmaskarray(block)
                excluding_mask = m if excluding_mask is None else (excluding_mask | m)
        blockx, blocky = [np.asarray(np.ma.getdata(b), dtype=np.float64) for b in (blockx, blocky)]
        mask = pnpoly(blockx, blocky, self.xseq, self.yseq, prev=previous_mask, mode=self.mode)
        if excluding_mask is not None:
            mask = mask & (~excluding_mask)
        return mask

    def _evaluate_device(self, df, i1, i2):
        from .superutils import pnpoly
        previous_mask = self.previous_selection.evaluate_device(df, i1, i2) if self.previous_selection else None
        blocks = []
        for expression in self.expressions:
            if df.data_type(expression) not in (np.dtype(np.float64), np.dtype(np.float32)):
                expression = "astype(%s, 'float64')" % expression  # the cast runs on the device too
            block = df._eval_host(expression, i1, i2)
            if np.ma.isMaskedArray(block):
                raise NotImplementedError("a lasso over a masked host column of an HBM frame")
            if not isinstance(block, DeviceArray):  # a host column of a mixed frame
                block = DeviceArray.from_numpy(np.ascontiguousarray(block))
            blocks.append(block)
        return pnpoly(blocks[0], blocks[1], self.xseq, self.yseq, prev=previous_mask, mode=self.mode)


class SelectionDropNa(Selection):
    def __init__(self, drop_nan, drop_masked, column_names, previous_selection, mode):
        _check_mode(mode)
        super(SelectionDropNa, self).__init__(previous_selection, mode)
        self.drop_nan = drop_nan
        self.drop_masked = drop_masked
        self.column_names = list(column_names)
        self.expressions = self.column_names

    def to_dict(self):
        return dict(type="dropna", drop_nan=self.drop_nan, drop_masked=self.drop_masked, column_names=self.column_names,
                    mode=self.mode, previous_selection=self._previous_dict())

    def _own_expression(self, df):
        """On an HBM frame the node is the expression ``~isnan(a) & ~isnan(b) ...``, with a
        ``notmissing(c)`` term for every masked HBM column among them; on a host frame it has
        none (``np.ma`` columns are read node by node)."""
        if df is None or not df.is_device_resident():
            return None
        terms = ["~isnan(%s)" % name for name in self.column_names] if self.drop_nan else []
        if self.drop_masked:  # the masked HBM columns among them (DeviceMaskedArray)
            terms += ["notmissing(%s)" % name for name in self.column_names
                      if not np.ma.isMaskedArray(df.columns.get(name)) and df.is_masked(name)]
        return " & ".join(terms) if terms else "True"

    def fold(self, df=None):
        own = self._own_expression(df)
        return None if own is None else self._fold_mode(own, df)

    def _evaluate(self, df, i1, i2, filter_mask):
        """selections.py:77-101."""
        previous_mask = self._previous_mask(df, i1, i2, filter_mask)
        n = int(np.sum(filter_mask)) if filter_mask is not None else i2 - i1
        mask = np.ones(n, dtype=bool)
        for name in self.column_names:
            data = df._eval_host(name, i1, i2, filter_mask)
            if self.drop_masked and np.ma.isMaskedArray(data):
                mask &= ~np.ma.getmaskarray(data)
            if self.drop_nan and np.ma.getdata(data).dtype.kind == "f":
                mask &= ~np.isnan(np.ma.getdata(data))
        return _select_functions[self.mode](previous_mask, mask)


def selection_from_dict(values):
    kwargs = dict(values)
    del kwargs["type"]
    previous = values["previous_selection"]
    kwargs["previous_selection"] = selection_from_dict(previous) if previous else None
    types = {"lasso": SelectionLasso, "expression": SelectionExpression, "invert": SelectionInvert,
             "dropna": SelectionDropNa}
    if values["type"] not in types:
        raise ValueError("unknown type: %r, in dict: %r" % (values["type"], values))
    return types[values["type"]](**kwargs)
