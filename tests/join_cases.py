"""Data and the numpy reference shared by the join-probe tests (GPU routes and
CPU oracle): tiny dimensions whose keys sit where a probe goes wrong, and one
fact table per dimension whose keys are drawn from `dimension keys + near
misses`.

Fact geometry is test_interpreted_routes': batches of 2*1024 + 37 and
1024 + 1 rows (two staged chunks, a ragged tail, a one-row chunk).  Measures
are small integers held in doubles, so every sum is exact in a double whatever
order the atomics land in, and every assertion downstream is `==`.

The contract the reference states (join section): a row joins when
its key is NOT NULL and equal to a dimension key; NULL keys join on neither
side; INT64_MIN is not a legal dimension key and, as a fact key, never joins.

Fact columns: measures D0, D1; G3 (three values, the fact half of the
`attr x fact_col` grouping); F, a nullable double every plan only filters on
(one real NULL in batch 1 of the INTERPRETED variant keeps a plan off the
query-compiled kernels; the COMPILED variant has none); the key columns K32,
K64 and the nullable KN64, KN32 (about 15 % NULL in both batches, each NULL
slot holding a 0)."""
import numpy as np

from oracle import pyoracle as po

(C_D0, C_D1, C_G3, C_F, C_K32, C_K64, C_KN64, C_KN32) = range(8)
DTYPES = [po.T_DOUBLE, po.T_DOUBLE, po.T_INT32, po.T_DOUBLE, po.T_INT32,
          po.T_INT64, po.T_INT64, po.T_INT32]
NULLABLE = [c in (C_F, C_KN64, C_KN32) for c in range(8)]
SCHEMA = list(zip(DTYPES, NULLABLE))

SIZES = (2 * 1024 + 37, 1024 + 1)
N = sum(SIZES)
NULL_F_ROW = SIZES[0] + 500
F_PRED = dict(col=C_F, is_double=True, lo=0.0)

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
LUT_MAX_SPAN = 1 << 24            # sn_lut_span's bound
SLUT_MAX_SPAN = 204800            # nibble LUT: span / 8 words * 4 B <= 100 KiB

M64 = (1 << 64) - 1


# ------------------------------------------------- the engine's hash, mirrored


def mix64(x):
    """splitmix64 finaliser: engine.cpp mix64h == kernels.hip mix64 ==
    the query-compiled probe's mix64."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def home(key, cap):
    """first slot probed for `key` in a table of `cap` slots (the kernels
    truncate the hash to 32 bits, then mask)."""
    return (mix64(key & M64) & 0xFFFFFFFF) & (cap - 1)


def put_cap(n):
    """slots of a sn_dim_put table of n keys: the smallest power of two that
    is at least 2n + 1."""
    lg = 1
    while (1 << lg) < 2 * n + 1:
        lg += 1
    return 1 << lg


def build_cap(rows):
    """slots of a k_join_build table: at least 1024 and at least 2 * rows."""
    lg = 10
    while (1 << lg) < 2 * rows and lg < 25:
        lg += 1
    return 1 << lg


def occupied(keys, cap):
    """{slot: key} after linear-probe insertion in the given order (the slot
    SET does not depend on the order, so it also holds for the device build,
    whose insertion order is not defined)."""
    slots = {}
    for k in keys:
        h = home(k, cap)
        while h in slots:
            h = (h + 1) & (cap - 1)
        slots[h] = k
    return slots


def _chain_set(cap, nkeys, seed_key):
    """nkeys keys of span > 2^24 for a table of `cap` slots: four whose home
    slots are the last two, so their chain occupies cap-2, cap-1, 0, 1 (it
    wraps), the rest homed in [8, cap-8) with slot 2 left empty; and four
    absent keys homed at cap-2, cap-1, 0, 1, which walk the chain to the empty
    slot 2 and miss.  Candidates are seed_key + i * 2^25."""
    want = {cap - 2: 2, cap - 1: 2}
    chain, rest, miss_homes, misses = [], [], [cap - 2, cap - 1, 0, 1], []
    i = 0
    while want or len(rest) < nkeys - 4 or miss_homes:
        k = seed_key + i * (1 << 25)
        i += 1
        h = home(k, cap)
        if want.get(h):
            chain.append(k)
            want[h] -= 1
            if not want[h]:
                del want[h]
        elif h in miss_homes:
            misses.append(k)
            miss_homes.remove(h)
        elif 8 <= h < cap - 8 and len(rest) < nkeys - 4:
            rest.append(k)
        assert i < 1 << 20
    return chain + rest, misses


def check_chain(keys, misses, cap):
    """the precondition the chain cases rest on; fails when the hash or the
    capacity rule changes, instead of the coverage going quietly"""
    slots = occupied(keys, cap)
    chain = keys[:4]
    assert all(home(k, cap) >= cap - 2 for k in chain)
    assert {s for s, k in slots.items() if k in chain} == {cap - 2, cap - 1, 0, 1}
    assert 2 not in slots                      # where every walk below ends
    assert sorted(home(k, cap) for k in misses) == [0, 1, cap - 2, cap - 1]
    assert not set(misses) & set(keys)
    assert max(keys) - min(keys) + 1 > LUT_MAX_SPAN


# ------------------------------------------------------------ dimension sets


class DimSet:
    """keys (python ints, unique), the attribute ordinal of each key, and the
    absent keys the fact table also draws."""

    def __init__(self, name, keys, near, nattr=4, attr_of=None):
        assert len(set(keys)) == len(keys) and not set(near) & set(keys)
        self.name = name
        self.keys = [int(k) for k in keys]
        self.near = [int(k) for k in near]
        self.nattr = nattr
        self.attr_ord = [attr_of(i) if attr_of else i % nattr
                         for i in range(len(keys))]

    def attrs(self, nattr=None):
        """attribute bytes per key; nattr re-deals the ordinals i % nattr"""
        if nattr is None:
            return [b"A%03d" % a for a in self.attr_ord]
        return [b"A%03d" % (i % nattr) for i in range(len(self.keys))]

    def key_cols(self):
        """the fact key columns that can meet this dimension (the int32
        columns only when a dimension key fits one)"""
        if any(I32_MIN <= k <= I32_MAX for k in self.keys):
            return (C_K32, C_K64, C_KN64, C_KN32)
        return (C_K64, C_KN64)

    @property
    def span(self):
        return max(self.keys) - min(self.keys) + 1

    @property
    def lut(self):
        """does sn_lut_span give this key range a dense LUT?"""
        return self.span <= LUT_MAX_SPAN


def _near(keys, extra=()):
    out = []
    for k in list(keys):
        for d in (-1, 1):
            if I64_MIN <= k + d <= I64_MAX:
                out.append(k + d)
    out += list(extra)
    return sorted(set(out) - set(keys))


_WIDE = [0, -1, 7, -(1 << 40), (1 << 24) + 1, (1 << 53) + 1, 1 << 62,
         -(1 << 62), I64_MAX, I64_MIN + 1, 12345678901, -77]
# I64_MIN + 1 - 1 is the empty-slot mark itself: a fact value that must miss
HASH_WIDE = DimSet("hash_wide", _WIDE, _near(_WIDE))
assert I64_MIN in HASH_WIDE.near and not HASH_WIDE.lut

_ck, _cm = _chain_set(put_cap(12), 12, 1 << 33)
HASH_CHAIN = DimSet("hash_chain", _ck, _cm)
check_chain(HASH_CHAIN.keys, HASH_CHAIN.near, put_cap(12))

# the same property at k_join_build's capacity (a build table of 12 rows)
_bk, _bm = _chain_set(build_cap(12), 12, -(1 << 45))
BUILD_CHAIN = DimSet("build_chain", _bk, _bm)
check_chain(BUILD_CHAIN.keys, BUILD_CHAIN.near, build_cap(12))


def lut_edge(span, lmin):
    lmax = lmin + span - 1
    inner = [lmin + 7, lmin + 8, lmin + span // 3, lmin + span // 2]
    if lmin < 0 < lmax and 0 not in inner:
        inner.append(0)
    keys = [lmin, lmin + 1] + inner + [lmax - 1, lmax]
    near = [lmin - 1, lmax + 1, lmin + 2, lmax - 2, lmin + span // 2 + 1,
            1 << 40, -(1 << 40), I64_MAX]
    return DimSet("lut_%d_%d" % (span, lmin), keys, near)


LUT_EDGES = {p: lut_edge(*p) for p in [
    (204800, -100000), (204801, -100000), (204793, 3),
    (1 << 24, -(1 << 23)), ((1 << 24) + 1, 0)]}
assert [d.lut for d in LUT_EDGES.values()] == [True] * 4 + [False]
assert 0 in LUT_EDGES[(204800, -100000)].keys


def _attr_set(name, n, step=10):
    """2n keys step apart, n attributes in order of first use, so attribute
    ordinal == the engine's gid and the highest gid sits on the largest key"""
    keys = [5 + step * i for i in range(2 * n)]
    d = DimSet(name, keys, _near(keys), nattr=n)
    assert d.attr_ord[-1] == n - 1 and d.attr_ord[:n] == list(range(n))
    return d


ATTR14 = _attr_set("attr14", 14)
ATTR15 = _attr_set("attr15", 15)
ATTR25 = _attr_set("attr25", 25)
# attr x G3 beyond the 1024-row result page: the global-accumulator routes
BIG_LUT = DimSet("big_lut", [3 * i for i in range(350)],
                 [3 * i + 1 for i in range(40)], nattr=350)
BIG_HASH = DimSet("big_hash", [i << 20 for i in range(350)],
                  [(i << 20) + 1 for i in range(40)], nattr=350)
assert BIG_LUT.lut and not BIG_HASH.lut and 350 * 3 > 1024

# extreme span (the LUT span arithmetic): {-(2^62), 0, 2^62}
EXTREME = DimSet("extreme", [-(1 << 62), 0, 1 << 62],
                 [-(1 << 62) + 1, 1, -1, (1 << 62) - 1, I64_MAX, I64_MIN])

DIMSETS = {d.name: d for d in
           [HASH_WIDE, HASH_CHAIN, BUILD_CHAIN, ATTR14, ATTR15, ATTR25,
            BIG_LUT, BIG_HASH, EXTREME] + list(LUT_EDGES.values())}


# ---------------------------------------------------------------- fact data


class Fact:
    """fact columns for one dimension set: cols[c] numpy arrays, valid[c]
    bool arrays (NULL slots hold a 0)."""

    def __init__(self, dim, interpreted):
        rng = np.random.default_rng(
            2085 + sum(dim.name.encode()) * 7 + len(dim.keys))
        self.dim, self.interpreted = dim, interpreted
        pool64 = dim.keys + dim.near
        pool32 = [k for k in pool64 if I32_MIN <= k <= I32_MAX] or [0]
        # every pool value at least once, the rest drawn with dimension keys
        # twice as likely as near misses
        def draw(pool):
            w = np.array([2.0 if k in set(dim.keys) else 1.0 for k in pool])
            ix = rng.choice(len(pool), size=N, p=w / w.sum())
            ix[rng.permutation(N)[:len(pool)]] = np.arange(len(pool))
            return [pool[i] for i in ix]
        cols = {
            C_D0: rng.integers(0, 8, N).astype(np.float64),
            C_D1: rng.integers(0, 8, N).astype(np.float64),
            C_G3: (np.arange(N) * 2 % 3).astype(np.int32),
            C_F: rng.integers(1, 4, N).astype(np.float64),
            C_K32: np.array(draw(pool32), dtype=np.int32),
            C_K64: np.array(draw(pool64), dtype=np.int64),
            C_KN64: np.array(draw(pool64), dtype=np.int64),
            C_KN32: np.array(draw(pool32), dtype=np.int32),
        }
        valid = {c: np.ones(N, dtype=bool) for c in range(8)}
        if interpreted:
            valid[C_F][NULL_F_ROW] = False
        for c in (C_KN64, C_KN32):
            valid[c] = rng.random(N) >= 0.15
            for s, e in self.bounds():          # NULLs in both batches
                assert not valid[c][s:e].all()
        for c in cols:
            cols[c] = np.where(valid[c], cols[c], 0).astype(cols[c].dtype)
        self.cols, self.valid = cols, valid

    @staticmethod
    def bounds():
        s = 0
        for n in SIZES:
            yield s, s + n
            s += n


_FACTS = {}


def fact(dim, interpreted):
    key = (dim.name, bool(interpreted))
    if key not in _FACTS:
        _FACTS[key] = Fact(dim, interpreted)
    return _FACTS[key]


# ---------------------------------------------------------------- reference

SUM = lambda c: ("sum", [(c, 0.0, 1.0)])            # noqa: E731
COUNT = ("count", [])
AGGS = [SUM(C_D0), COUNT]
# seven aggregates: past k_grouped_reg's six, the plan takes k_grouped
AGGS7 = [SUM(C_D0), SUM(C_D1), ("sum", [(C_D0, 1.0, 1.0)]),
         ("sum", [(C_D1, 0.0, 2.0)]), ("sum", [(C_D0, 0.0, 1.0), (C_D1, 0.0, 1.0)]),
         ("sum", [(C_D0, 2.0, 1.0)]), COUNT]

MODES = ("semi", "semi_g3", "attr", "attr_g3")


def plan_args(mode, key_col, dim_handle, aggs=AGGS):
    """keyword arguments of abi.make_plan / pyoracle.make_plan (minus table)"""
    return dict(preds=[F_PRED], aggs=aggs,
                group_cols=[C_G3] if mode.endswith("_g3") else [],
                join=dict(dim=dim_handle, fact_col=key_col,
                          group=mode.startswith("attr")))


def agg_rows(fx, agg):
    """per-row contribution of a SUM (product of its factors) or COUNT: small
    integers, so summing them in any order is exact"""
    kind, factors = agg
    assert kind in ("sum", "count")
    v = np.ones(N)
    for col, add, mul in factors:
        v = v * (add + mul * fx.cols[col])
    return v


def reference(fx, key_col, dim_keys, dim_attrs, mode, aggs=AGGS):
    """{key tuple: [aggregate values]} of the join of fact `fx` on key_col
    with the dimension {dim_keys[i]: dim_attrs[i]} (attrs bytes; ignored by
    the semi modes):  joined = valid(key) & isin(key, dim)."""
    attr_of = {int(k): (a.decode() if a is not None else None)
               for k, a in zip(dim_keys, dim_attrs or [None] * len(dim_keys))}
    keys = fx.cols[key_col]
    joined = fx.valid[key_col] & fx.valid[C_F] & \
        np.array([int(k) in attr_of for k in keys])
    parts = []
    if mode.startswith("attr"):
        parts.append(np.array([attr_of.get(int(k)) for k in keys], dtype=object))
    if mode.endswith("_g3"):
        parts.append(np.array([str(int(g)) for g in fx.cols[C_G3]], dtype=object))
    assert joined.any()
    vals = [agg_rows(fx, a) for a in aggs]
    out = {}
    for r in np.nonzero(joined)[0]:
        acc = out.setdefault(tuple(p[r] for p in parts), [0.0] * len(aggs))
        for a, v in enumerate(vals):
            acc[a] += float(v[r])
    return out


# ------------------------------------------------------------- build tables


class Build:
    """a build-side column table for sn_dim_from_table: one batch of key
    (+ attribute) rows, with optional NULL keys, deleted rows and a put-time
    update delta on the key column.  effective() is the dimension it means."""

    def __init__(self, name, keys, attr_ord, key_type=po.T_INT64, valid=None,
                 deleted=(), patch=None, how="raw", stats=None):
        self.name, self.key_type = name, key_type
        self.keys = [int(k) for k in keys]
        self.attrs = [b"B%03d" % a for a in attr_ord]
        self.valid = [True] * len(keys) if valid is None else list(valid)
        self.deleted = sorted(deleted)
        self.patch = dict(patch or {})          # row -> new key
        self.how = how        # "raw": ingest_columns; "encoded": batch_put
        self.stats = stats    # (lo, hi) of the key column's stats row

    def effective(self):
        keys, attrs = [], []
        for r, (k, a, ok) in enumerate(zip(self.keys, self.attrs, self.valid)):
            k = self.patch.get(r, k)
            if not ok or r in self.deleted:
                continue
            if k in keys:
                assert attrs[keys.index(k)] == a    # same attribute: accepted
                continue
            keys.append(k)
            attrs.append(a)
        return keys, attrs


_E = LUT_EDGES[(204793, 3)]
BUILDS = {b.name: b for b in [
    # raw int64 ingest -> device stats: narrow span -> LUT
    Build("raw_narrow", _E.keys, _E.attr_ord),
    # ... wide span -> hash, with a wrapping chain at k_join_build's capacity
    Build("raw_wide", BUILD_CHAIN.keys, BUILD_CHAIN.attr_ord),
    # encoded put without a stats row: no bounds -> hash even for narrow keys
    Build("encoded_nostats", _E.keys, _E.attr_ord, how="encoded"),
    # NULL build keys never join: their slot holds a 0, and 0 is a fact key
    Build("null_keys", [0, 0, 5, 15, 0, 25, 35], [0, 1, 1, 2, 3, 0, 1],
          valid=[False, False, True, True, False, True, True]),
    # deleted build rows never join
    Build("deleted", ATTR14.keys, ATTR14.attr_ord, how="encoded",
          deleted=[0, 3, 27]),
    # duplicate keys carrying the same attribute are accepted
    Build("dup_same_attr", ATTR14.keys + ATTR14.keys[:6],
          ATTR14.attr_ord + ATTR14.attr_ord[:6]),
    # extreme span: signed span arithmetic wraps on these
    Build("extreme", EXTREME.keys, [0, 1, 2]),
    # stale bounds: the stats row says [0, 99], a put-time delta moves the
    # key of row 2 to 5000
    Build("stale_bounds", [10 * i + 5 for i in range(10)], [i % 3 for i in range(10)],
          how="encoded", stats=(0, 99), patch={2: 5000}),
]}
# the fact table each build is probed by (its dimension set supplies the keys
# drawn), by build name
# null_keys and stale_bounds probe sets of their own: the surviving build
# keys, and as near misses the values a wrong build would join (the 0 of a
# NULL slot; the key 25 the delta patched away)
NULLB = DimSet("nullb", BUILDS["null_keys"].effective()[0], [0, 4, 6, 36])
STALE = DimSet("stale", BUILDS["stale_bounds"].effective()[0],
               [25, 0, 99, 100, 4999, 5001, 6])
assert NULLB.keys == [5, 15, 25, 35]
assert 25 not in STALE.keys and 5000 in STALE.keys
BUILD_FACT = {"raw_narrow": _E, "raw_wide": BUILD_CHAIN, "encoded_nostats": _E,
              "null_keys": NULLB, "deleted": ATTR14, "dup_same_attr": ATTR14,
              "extreme": EXTREME, "stale_bounds": STALE}
DIMSETS.update({NULLB.name: NULLB, STALE.name: STALE})
