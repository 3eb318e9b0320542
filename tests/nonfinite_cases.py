"""Data, plans and the reference shared by the non-finite tests (GPU routes
and CPU oracle): one table whose aggregate inputs hold +-inf, NaN and
overflowing products at chosen rows, and the numpy statement of the contract
("Non-finite aggregate inputs").

Every finite value is a small integer held in a double, so every finite sum
is exact whatever the order of addition, and numpy's sum under
np.errstate(all="ignore") is an order-independent reference for SUM and AVG
with the specials in.  MIN/MAX follow ref_minmax below.

The filter column F decides which planted rows a plan sees:

   F     rows                                 SUM_PRED  JOIN_PRED  MM_PRED  ALL_PRED
  -9     the NULL row (NULL in interp)           -         -         -        -
  -1     fail rows (specials everywhere)         -         -         -        x
  0.25   join-miss rows (specials everywhere)    -         x         -        x
  0.5    passing specials of the SUM groups      x         x         -        x
  1..3   regular rows                            x         x         x        x
  4      rows of the MIN/MAX groups              -         -         x        x

In the delete-mask variant the fail rows carry F = 2 (they pass) and are
deleted instead.  Each planted row exists three times: inside a staged chunk
of batch 0, inside batch 0's ragged tail, and in the last batch."""
import numpy as np

from oracle import pyoracle as po

(C_F, C_V, C_W, C_X, C_A, C_B, C_G6, C_G12, C_G40, C_G1500, C_K64, C_JK,
 C_M6, C_M40, C_M1500, C_MK) = range(16)
NCOLS = 16

# oracle / engine type codes agree (T_DOUBLE == 2 ...)
DTYPES = [po.T_DOUBLE] * 3 + [po.T_FLOAT] + [po.T_DOUBLE] * 2 + \
         [po.T_INT32] * 4 + [po.T_INT64, po.T_INT32] + [po.T_INT32] * 3 + \
         [po.T_INT64]
NULLABLE = [c in (C_F, C_K64) for c in range(NCOLS)]

SIZES = (2 * 1024 + 37, 1024 + 1)      # test_interpreted_routes' geometry
RADIX_SIZES = (40_000,)                # > 32,768 rows: cap_log2 stays >= 17
SPARSE_KEYS = 48                       # + the -1 key + the NULL key = 50
RADIX_KEYS = 3000

INF = np.inf
NAN_POS = np.uint64(0x7FF8000000000000)
NAN_NEG = np.uint64(0xFFF8000000000000)
NAN_PAYLOAD = np.uint64(0x7FF8000000000001)


def _bits(u):
    return np.array([u], dtype=np.uint64).view(np.float64)[0]


F_NULL, F_FAIL, F_MISS, F_SPECIAL, F_MM = -9.0, -1.0, 0.25, 0.5, 4.0

SUM_PRED = dict(col=C_F, is_double=True, lo=0.4, hi=3.5)
JOIN_PRED = dict(col=C_F, is_double=True, lo=0.0, hi=3.5)
MM_PRED = dict(col=C_F, is_double=True, lo=0.9, hi=5.0)
ALL_PRED = dict(col=C_F, is_double=True, lo=-5.0)

# planted kinds: (F, V, W, X, A, B, SUM group, MIN/MAX group)
#   SUM groups: 1 +inf only, 2 +inf and -inf, 3 W = NaN, 4 A*B overflows;
#               0 and 5 stay finite
#   MIN/MAX groups: 0 finite + NaN (sign clear), 1 finite + NaN (sign set),
#               2 all NaN, 3 {-inf, finite, +inf}, 4 {-0.0, +0.0}, 5 finite,
#               6 finite + a NaN in the last batch only (so that a merge of
#               per-batch partials meets a NaN on one side alone)
_NP, _NN, _NQ = _bits(NAN_POS), _bits(NAN_NEG), _bits(NAN_PAYLOAD)
PLANTED = [
    ("fail", F_FAIL, INF, _NP, INF, 1e200, 1e200, 0, 5),
    ("miss", F_MISS, INF, _NP, INF, 1e200, 1e200, 0, 5),
    ("inf", F_SPECIAL, INF, 1.0, INF, 1.0, 1.0, 1, 5),
    ("pinf", F_SPECIAL, INF, 1.0, 1.0, 1.0, 1.0, 2, 5),
    ("ninf", F_SPECIAL, -INF, 1.0, 1.0, 1.0, 1.0, 2, 5),
    ("wnan", F_SPECIAL, 1.0, _NP, 1.0, 1.0, 1.0, 3, 5),
    ("ab", F_SPECIAL, 1.0, 1.0, 1.0, 1e200, 1e200, 4, 5),
    ("mm_nanpos", F_MM, _NP, _NP, _NP, 1.0, 1.0, 0, 0),
    ("mm_nanneg", F_MM, _NN, _NN, _NN, 1.0, 1.0, 0, 1),
    ("mm_all_a", F_MM, _NP, _NP, _NP, 1.0, 1.0, 0, 2),
    ("mm_all_b", F_MM, _NN, _NN, _NN, 1.0, 1.0, 0, 2),
    ("mm_all_c", F_MM, _NQ, _NQ, _NQ, 1.0, 1.0, 0, 2),
    ("mm_ninf", F_MM, -INF, -INF, -INF, 1.0, 1.0, 0, 3),
    ("mm_pinf", F_MM, INF, INF, INF, 1.0, 1.0, 0, 3),
    ("mm_nzero", F_MM, -0.0, -0.0, -0.0, 1.0, 1.0, 0, 4),
    ("mm_pzero", F_MM, 0.0, 0.0, 0.0, 1.0, 1.0, 0, 4),
    ("mm_nan_last", F_MM, _NP, _NP, _NP, 1.0, 1.0, 0, 6),
]
ONLY_LAST = ("mm_nan_last",)           # planted in the last region alone
MM_REGULAR = (0, 1, 3, 5, 6)           # MIN/MAX groups that hold regular rows

# dimension of the join cases: the even keys, six attribute values; planted
# passing rows of SUM group g join through key 2*g, the join-miss rows hold
# an odd key
DIM_KEYS = np.arange(0, 100, 2, dtype=np.int64)
DIM_ATTRS = [b"A%d" % (int(k) // 2 % 6) for k in DIM_KEYS]


class Data:
    """cols[c] (numpy arrays over all batches), valid[c], deleted, sizes."""

    def __init__(self, sizes, nkeys, nulls, deletes):
        self.sizes = tuple(sizes)
        self.n = n = sum(sizes)
        self.nkeys = nkeys
        rng = np.random.default_rng(4177)
        i = np.arange(n)
        cols = {}
        valid = {c: np.ones(n, dtype=bool) for c in range(NCOLS)}
        cols[C_F] = rng.integers(1, 4, n).astype(np.float64)
        cols[C_V] = rng.integers(0, 1000, n).astype(np.float64)
        cols[C_W] = rng.integers(0, 8, n).astype(np.float64)
        cols[C_X] = rng.integers(0, 8, n).astype(np.float32)
        cols[C_A] = rng.integers(0, 8, n).astype(np.float64)
        cols[C_B] = rng.integers(0, 8, n).astype(np.float64)
        g = {C_G6: i % 6, C_G12: i * 5 % 12, C_G40: i * 7 % 40,
             C_G1500: i * 7 % 1500}
        kidx = i * 13 % (nkeys + 2)
        cols[C_JK] = rng.integers(0, 100, n).astype(np.int32)
        mm = np.array(MM_REGULAR)[i % 5]

        # plant: kind j sits at one row of each region
        last = sum(sizes[:-1])
        if len(sizes) > 1:
            regions = (100, 2 * 1024, last + 50)
            strides = (37, 1, 29)
        else:                         # one batch: tile 0, tile 1, the tail
            regions = (1000, 16384 + 500, n - 64)
            strides = (37, 41, 1)
        self.deleted = np.zeros(n, dtype=bool)
        self.planted_rows = {}
        for j, (name, f, v, w, x, a, b, sg, mg) in enumerate(PLANTED):
            rows = [r0 + j * st for r0, st in zip(regions, strides)]
            if name in ONLY_LAST:
                rows = rows[-1:]
            self.planted_rows[name] = rows
            for r in rows:
                cols[C_F][r] = f
                cols[C_V][r], cols[C_W][r] = v, w
                cols[C_X][r] = np.float32(x)
                cols[C_A][r], cols[C_B][r] = a, b
                for c in g:
                    g[c][r] = sg
                kidx[r] = sg
                mm[r] = mg
                cols[C_JK][r] = 1 if name == "miss" else 2 * sg
                if name == "fail" and deletes:
                    cols[C_F][r] = 2.0
                    self.deleted[r] = True
        assert max(max(r) for r in self.planted_rows.values()) < n
        assert self.planted_rows["mm_pzero"][1] < sizes[0]

        for c in g:
            cols[c] = g[c].astype(np.int32)
        k64 = kidx.astype(np.int64) * (1 << 33) + 12345
        k64[kidx == nkeys] = -1
        cols[C_K64] = k64
        cols[C_M6] = mm.astype(np.int32)
        cols[C_M40] = (mm * 7).astype(np.int32)
        cols[C_M1500] = (mm * 299).astype(np.int32)
        cols[C_MK] = mm.astype(np.int64) * (1 << 33) + 12345

        # the one row that keeps the interp table off the compiled kernels:
        # it fails every predicate, as a NULL there and as F_NULL here
        self.null_f_row = last + 500 if len(sizes) > 1 else 777
        assert self.null_f_row not in sum(self.planted_rows.values(), [])
        cols[C_F][self.null_f_row] = F_NULL
        if nulls:
            valid[C_F][self.null_f_row] = False
            valid[C_K64][kidx == nkeys + 1] = False
        self.cols, self.valid = cols, valid

    def batches(self):
        """(start, n) of each batch"""
        s = 0
        for n in self.sizes:
            yield s, n
            s += n

    def stats(self, start, n):
        """the batch's stats row: bounds over the non-NULL values, a float
        column's over its non-NaN ones (what the put-time bounds hold)"""
        lo, hi, nulls = [], [], []
        for c in range(NCOLS):
            ok = self.valid[c][start:start + n]
            x = self.cols[c][start:start + n][ok]
            if x.dtype.kind == "f":
                x = x[~np.isnan(x)].astype(np.float64)
            lo.append(x.min())
            hi.append(x.max())
            nulls.append(int(n - ok.sum()))
        return po.encode_stats(DTYPES, n, lo, hi, null_counts=nulls)

    def delete_positions(self, start, n):
        d = np.nonzero(self.deleted[start:start + n])[0]
        return d.astype(np.int32)


_DATA = {}


def data(kind):
    """'clean', 'interp', 'clean_del', 'interp_del', 'radix' (built once)"""
    if kind not in _DATA:
        if kind == "radix":
            _DATA[kind] = Data(RADIX_SIZES, RADIX_KEYS, False, False)
        else:
            _DATA[kind] = Data(SIZES, SPARSE_KEYS, kind.startswith("interp"),
                               kind.endswith("_del"))
    return _DATA[kind]


# ------------------------------------------------------------------ plans

SUM = lambda c: ("sum", [(c, 0.0, 1.0)])            # noqa: E731
AVG = lambda c: ("avg", [(c, 0.0, 1.0)])            # noqa: E731
MIN = lambda c: ("min", [(c, 0.0, 1.0)])            # noqa: E731
MAX = lambda c: ("max", [(c, 0.0, 1.0)])            # noqa: E731
SUM_AB = ("sum", [(C_A, 0.0, 1.0), (C_B, 0.0, 1.0)])
COUNT = ("count", [])

SUM_AGGS = [SUM(C_V), SUM(C_W), AVG(C_V), SUM_AB, COUNT]
SUM_AGGS4 = [SUM(C_V), SUM(C_W), SUM_AB, COUNT]     # radix: <= 4 aggregates
WBIN_AGGS = [SUM(C_V), COUNT]                       # wbin: <= 2 aggregates
MM_AGGS = [MIN(C_V), MAX(C_V), MIN(C_W), MAX(C_W), MAX(C_X), COUNT]
MM_AGGS4 = [MIN(C_V), MAX(C_V), MAX(C_W), COUNT]


# -------------------------------------------------------------- reference


def ref_minmax(kind, x):
    """The contract: NaN (any sign, any payload) equals NaN and is greater
    than every other value, +inf included."""
    x = np.asarray(x, dtype=np.float64)
    nan = np.isnan(x)
    if kind == "max":
        return float("nan") if nan.any() else float(x.max())
    rest = x[~nan]
    return float("nan") if rest.size == 0 else float(rest.min())


def same(a, b):
    """both NaN, or == (so -0.0 and +0.0 are interchangeable)"""
    if a is None or b is None:
        return a is None and b is None
    return (a != a and b != b) or a == b


def assert_same_groups(got, exp):
    assert sorted(got, key=repr) == sorted(exp, key=repr)
    bad = [(k, a, got[k][a], exp[k][a]) for k in exp
           for a in range(len(exp[k])) if not same(got[k][a], exp[k][a])]
    assert not bad, "(key, aggregate, got, expected): %r" % bad[:12]


def pred_mask(d, preds):
    m = ~d.deleted
    for p in preds:
        x = d.cols[p["col"]]
        m = m & d.valid[p["col"]]
        if "lo" in p:
            m = m & (x >= p["lo"])
        if "hi" in p:
            m = m & (x <= p["hi"])
    return m


def agg_values(d, aggs, m):
    out = []
    with np.errstate(all="ignore"):
        for kind, factors in aggs:
            if kind == "count":
                out.append(float(m.sum()))
                continue
            v = np.ones(d.n)
            for col, add, mul in factors:
                assert d.valid[col][m].all()
                v = v * (add + mul * d.cols[col].astype(np.float64))
            x = v[m]
            assert len(x) > 0
            if kind in ("min", "max"):
                out.append(ref_minmax(kind, x))
            else:
                s = float(x.sum())
                out.append(s if kind == "sum" else s / len(x))
    return out


def int_keys(d, col):
    return np.array([str(int(v)) if ok else None
                     for v, ok in zip(d.cols[col], d.valid[col])], dtype=object)


def attr_keys(d):
    lut = {int(k): a.decode() for k, a in zip(DIM_KEYS, DIM_ATTRS)}
    return np.array([lut.get(int(k)) for k in d.cols[C_JK]], dtype=object)


def reference(d, case, rows=None):
    """{key tuple: [aggregate values]} of a CASES entry over the rows of the
    boolean mask `rows` (default: all)."""
    preds, group_cols, aggs, join = case
    mask = pred_mask(d, preds)
    if rows is not None:
        mask &= rows
    keycols = []
    if join is not None:
        akeys = attr_keys(d)
        mask &= np.array([a is not None for a in akeys])
        if join == "attr":
            keycols.append(akeys)
    keycols += [int_keys(d, c) for c in group_cols]
    if not keycols:
        return {(): agg_values(d, aggs, mask)}
    # group id per row, then one mask per distinct key
    ids, index = np.full(d.n, -1), {}
    for r in np.nonzero(mask)[0]:
        ids[r] = index.setdefault(tuple(k[r] for k in keycols), len(index))
    return {key: agg_values(d, aggs, ids == gi) for key, gi in index.items()}


# ----------------------------------------------------------------- oracle


def oracle_table(d):
    ot = po.OracleTable(DTYPES)
    for s, n in d.batches():
        blobs = []
        for c in range(NCOLS):
            v = d.valid[c][s:s + n]
            blobs.append(po.encode(
                DTYPES[c], po.ENC_UNCOMPRESSED, d.cols[c][s:s + n],
                valid=None if v.all() else v.astype(np.uint8)))
        dels = d.delete_positions(s, n)
        ot.add_batch(n, blobs, stats=d.stats(s, n),
                     delete_mask=po.encode_delete(dels, n)
                     if len(dels) else None)
    ot.set_dim(DIM_KEYS, DIM_ATTRS)
    return ot


def oracle_groups(ot, case, nthreads=1):
    preds, group_cols, aggs, join = case
    jspec = None if join is None else dict(dim=0, fact_col=C_JK,
                                           group=join == "attr")
    rows = ot.query_groups(po.make_plan(preds=preds, group_cols=group_cols,
                                        aggs=aggs, join=jspec),
                           nthreads=nthreads, cap=4096)
    got = {keys: vals for keys, vals in rows}
    assert len(got) == len(rows)
    return got


# id -> (preds, group cols, aggs, join: None | "semi" | "attr")
SUM_CASES = {
    "keyless_all_rows": ([ALL_PRED], [], SUM_AGGS, None),
    "keyless": ([SUM_PRED], [], SUM_AGGS, None),
    "regs_6slots": ([SUM_PRED], [C_G6], SUM_AGGS, None),
    "regs_6slots_4aggs": ([SUM_PRED], [C_G6], SUM_AGGS4, None),
    "grouped_12slots": ([SUM_PRED], [C_G12], SUM_AGGS, None),
    "wbin_6slots": ([SUM_PRED], [C_G6], WBIN_AGGS, None),
    "lds_40slots": ([SUM_PRED], [C_G40], SUM_AGGS, None),
    "global_1500slots": ([SUM_PRED], [C_G1500], SUM_AGGS, None),
    "sparse_int64_keys": ([SUM_PRED], [C_K64], SUM_AGGS, None),
    "join_group_attr": ([JOIN_PRED], [], SUM_AGGS, "attr"),
    "semi_join": ([JOIN_PRED], [], SUM_AGGS, "semi"),
}
RADIX_CASE = ([SUM_PRED], [C_K64], SUM_AGGS4, None)
RADIX_MM_CASE = ([MM_PRED], [C_MK], MM_AGGS4, None)

MM_CASES = {
    "mm_one_slot": ([MM_PRED], [], MM_AGGS, None),
    "mm_regs_7slots": ([MM_PRED], [C_M6], MM_AGGS, None),
    "mm_lds_43slots": ([MM_PRED], [C_M40], MM_AGGS, None),
    "mm_global_1800slots": ([MM_PRED], [C_M1500], MM_AGGS, None),
    "mm_sparse_int64_keys": ([MM_PRED], [C_MK], MM_AGGS, None),
}

# the delete-mask variant runs the routes whose accumulators see dead rows
DEL_CASES = ("keyless", "regs_6slots", "grouped_12slots", "lds_40slots",
             "mm_regs_7slots")
