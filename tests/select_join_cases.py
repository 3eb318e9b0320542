"""The numpy reference of the join row scans (sn_scan_submit_join), over the
data of tests/join_cases.py: its dimension sets, its fact tables
(fact(dim, interpreted): batches of 2*1024 + 37 and 1024 + 1 rows) and its
filter F_PRED.

With  passed = valid[C_F] & (F >= 0)  and  joined = valid[key] & isin(key,
dimension keys), the row sets are

    INNER        passed & joined
    LEFT_OUTER   passed
    LEFT_ANTI    passed & ~joined

in table order (batch, then ordinal).  Everything downstream compares bytes
with `==`."""
import numpy as np

from snappydata_amd import abi
from tests import join_cases as jc

INNER, OUTER, ANTI = abi.RJOIN_INNER, abi.RJOIN_LEFT_OUTER, abi.RJOIN_LEFT_ANTI
TYPES = (INNER, OUTER, ANTI)
TYPE_NAMES = {INNER: "inner", OUTER: "outer", ANTI: "anti"}


def projection(jtype, key_col):
    """what every case projects; LEFT_ANTI has no right side to project"""
    cols = [abi.PROJ_ROWID, jc.C_D0, key_col]
    return cols if jtype == ANTI else cols + [abi.PROJ_DIM_ATTR]


class Table:
    """the columns a reference needs, as the table holds them NOW: cols[c]
    (NULL slots hold 0), valid[c], deleted (bool per row), and the batch
    bounds.  from_fact is join_cases' fact table as loaded."""

    def __init__(self, cols, valid, bounds, deleted=None):
        self.cols = {c: np.array(v) for c, v in cols.items()}
        self.valid = {c: np.array(v) for c, v in valid.items()}
        self.bounds = list(bounds)
        n = self.bounds[-1][1]
        self.deleted = np.zeros(n, dtype=bool) if deleted is None else deleted
        rowid = np.zeros(n, dtype=np.int64)
        for bi, (s, e) in enumerate(self.bounds):
            rowid[s:e] = (bi << 32) | np.arange(e - s, dtype=np.int64)
        self.rowid = rowid

    @classmethod
    def from_fact(cls, fx):
        return cls(fx.cols, fx.valid, fx.bounds())


def masks(tb, key_col, dim_keys):
    """(passed, joined) bool arrays over the table's rows"""
    passed = tb.valid[jc.C_F] & (tb.cols[jc.C_F] >= 0) & ~tb.deleted
    dk = np.array([int(k) for k in dim_keys], dtype=np.int64)
    joined = tb.valid[key_col] & np.isin(tb.cols[key_col].astype(np.int64), dk)
    return passed, joined


class Rows:
    """expected result columns of one join scan, in table order"""

    def __init__(self, tb, key_col, dim_keys, dim_attrs, jtype):
        passed, joined = masks(tb, key_col, dim_keys)
        self.passed, self.joined = passed, joined
        keep = {INNER: passed & joined, OUTER: passed,
                ANTI: passed & ~joined}[jtype]
        self.index = np.nonzero(keep)[0]
        ix = self.index
        self.rowid = tb.rowid[ix]
        self.d0 = tb.cols[jc.C_D0][ix]
        self.key = tb.cols[key_col][ix]
        self.key_valid = tb.valid[key_col][ix]
        self.attr_valid = joined[ix]
        attr_of = {int(k): a for k, a in zip(dim_keys, dim_attrs)}
        self.attr = [attr_of[int(k)] if j else None
                     for k, j in zip(self.key, self.attr_valid)]

    def __len__(self):
        return len(self.index)

    def take(self, order):
        """the same rows in another order (or a prefix): a shallow copy"""
        r = object.__new__(Rows)
        order = np.asarray(order, dtype=np.int64)
        r.passed, r.joined = self.passed, self.joined
        r.index = self.index[order]
        r.rowid, r.d0 = self.rowid[order], self.d0[order]
        r.key, r.key_valid = self.key[order], self.key_valid[order]
        r.attr_valid = self.attr_valid[order]
        r.attr = [self.attr[int(i)] for i in order]
        return r


def stable_order(values, valid, descending, nulls_first=None):
    """positions of a stable sort by (NULL class, value): Spark's default puts
    NULLs first ascending and last descending; equal keys keep their order"""
    if nulls_first is None:
        nulls_first = not descending
    n = len(values)
    v = np.asarray(values).astype(object)
    idx = sorted(range(n), key=lambda i: (
        (0 if nulls_first else 2) if not valid[i] else 1,
        0 if not valid[i] else (-v[i] if descending else v[i]), i))
    return np.array(idx, dtype=np.int64)
