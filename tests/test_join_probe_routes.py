"""Exact tests of the join probe, route by route (data and reference:
tests/join_cases.py).

A probe is one of three kinds, decided by the dimension's key span and the
plan (jit.cpp jit_classify; probe_sweep takes the LUT or the hash table):

  hash  open-address chain walk       span > 2^24, or no trusted bounds
  spay  dense LUT, register-staged    span <= 2^24
  slut  dense LUT packed to nibbles   span <= 204800 and (semi-join or at
        in LDS                        most 14 group slots)

Compiled cases run on a fresh engine with SN_JIT_DUMP set and assert that the
dumped source carries the expected probe's mark and neither of the others.
Interpreted cases (the table variant with one real NULL in the filter column)
assert used_jit() is false; which hand-written kernel they reach follows from
the plan's shape (engine_internal.h sn_dense_launch_of):

  k_keyless          semi-join, no group column
  k_grouped_reg      semi-join x G3 (3 slots, <= 6 aggregates)
  k_grouped          semi-join x G3 with 7 aggregates (jmode 0); group by
                     attribute with <= 16 slots (jmode 1: the slot image)
  k_grouped_lds      17..1024 slots
  k_grouped_global   more than 1024 slots
  (k_grouped_hash's probe is unreachable: a join with sparse group keys is
  rejected.)

Every result is compared with `==`: all sums are sums of small integers."""
import collections

import numpy as np
import pytest

from oracle import pyoracle as po
from snappydata_amd import abi, engine as se
from tests import join_cases as jc

pytestmark = pytest.mark.gpu

MARKS = {"slut": "slut[ix >> 3]", "spay": "= spay[r]", "hash": "jkeys[h]"}

E = jc.LUT_EDGES
Case = collections.namedtuple(
    "Case", "id src key_col mode probe nattr aggs", defaults=(None, None, jc.AGGS))
PUT, TABLE = "put", "table"

COMPILED = [
    # ---- nibble LUT at its span limit, negative lut_min, both key widths
    Case("slut_204800_k32_semi", (PUT, E[(204800, -100000)]), jc.C_K32, "semi", "slut"),
    Case("slut_204800_k64_attr", (PUT, E[(204800, -100000)]), jc.C_K64, "attr", "slut"),
    # one past it: the register-staged LUT
    Case("spay_204801_k64_semi", (PUT, E[(204801, -100000)]), jc.C_K64, "semi", "spay"),
    Case("spay_204801_k32_attr", (PUT, E[(204801, -100000)]), jc.C_K32, "attr", "spay"),
    # span % 8 == 1: the nibble pack's `ix < span` tail
    Case("slut_204793_k64_attr_g3", (PUT, E[(204793, 3)]), jc.C_K64, "attr_g3", "slut"),
    Case("slut_204793_k32_semi_g3", (PUT, E[(204793, 3)]), jc.C_K32, "semi_g3", "slut"),
    # the largest LUT, and one key more: hash
    Case("spay_2p24_k64_attr", (PUT, E[(1 << 24, -(1 << 23))]), jc.C_K64, "attr", "spay"),
    Case("spay_2p24_k32_semi", (PUT, E[(1 << 24, -(1 << 23))]), jc.C_K32, "semi", "spay"),
    Case("hash_2p24p1_k64_attr", (PUT, E[((1 << 24) + 1, 0)]), jc.C_K64, "attr", "hash"),
    # 14 group slots fit a nibble (15 = absent), 15 do not
    Case("slut_attr14_k32", (PUT, jc.ATTR14), jc.C_K32, "attr", "slut"),
    Case("spay_attr15_k32", (PUT, jc.ATTR15), jc.C_K32, "attr", "spay"),
    Case("spay_attr14_x_g3_k64", (PUT, jc.ATTR14), jc.C_K64, "attr_g3", "spay"),
    # LDS and global accumulators
    Case("spay_attr25_k64", (PUT, jc.ATTR25), jc.C_K64, "attr", "spay"),
    Case("hash_big_k64_attr_g3", (PUT, jc.BIG_HASH), jc.C_K64, "attr_g3", "hash"),
    # ---- hash: extreme keys, the empty mark as a fact key, wrapping chains
    Case("hash_wide_k64_semi", (PUT, jc.HASH_WIDE), jc.C_K64, "semi", "hash"),
    Case("hash_wide_k64_attr", (PUT, jc.HASH_WIDE), jc.C_K64, "attr", "hash"),
    Case("hash_wide_k32_attr_g3", (PUT, jc.HASH_WIDE), jc.C_K32, "attr_g3", "hash"),
    Case("hash_chain_k64_attr", (PUT, jc.HASH_CHAIN), jc.C_K64, "attr", "hash"),
    Case("hash_chain_k64_semi_g3", (PUT, jc.HASH_CHAIN), jc.C_K64, "semi_g3", "hash"),
    Case("hash_extreme_put_k64_semi", (PUT, jc.EXTREME), jc.C_K64, "semi", "hash"),
    # ---- dimensions built on the device from a column table
    Case("table_raw_narrow_slut", (TABLE, "raw_narrow"), jc.C_K64, "attr", "slut"),
    Case("table_raw_wide_hash", (TABLE, "raw_wide"), jc.C_K64, "attr", "hash"),
    Case("table_encoded_nostats_hash", (TABLE, "encoded_nostats"), jc.C_K32, "attr", "hash"),
    Case("table_dup_same_attr_slut", (TABLE, "dup_same_attr"), jc.C_K32, "attr", "slut"),
    Case("table_deleted_hash", (TABLE, "deleted"), jc.C_K32, "attr", "hash"),
    Case("table_extreme_hash", (TABLE, "extreme"), jc.C_K64, "attr", "hash"),
    Case("table_stale_bounds_hash", (TABLE, "stale_bounds"), jc.C_K32, "attr", "hash"),
]

INTERPRETED = [
    # k_keyless
    Case("keyless_hash", (PUT, jc.HASH_WIDE), jc.C_K64, "semi"),
    Case("keyless_lut", (PUT, E[(204800, -100000)]), jc.C_K32, "semi"),
    # k_grouped_reg
    Case("reg_hash", (PUT, jc.HASH_CHAIN), jc.C_K64, "semi_g3"),
    Case("reg_lut", (PUT, E[(204793, 3)]), jc.C_K64, "semi_g3"),
    # k_grouped, jmode 0 (seven aggregates are past k_grouped_reg)
    Case("grouped_semi_hash", (PUT, jc.HASH_WIDE), jc.C_K64, "semi_g3", None, None, jc.AGGS7),
    Case("grouped_semi_lut", (PUT, E[(204801, -100000)]), jc.C_K32, "semi_g3", None, None, jc.AGGS7),
    # k_grouped, jmode 1: the slot image
    Case("grouped_attr_hash", (PUT, jc.HASH_WIDE), jc.C_K32, "attr"),
    Case("grouped_attr_g3_hash", (PUT, jc.HASH_CHAIN), jc.C_K64, "attr_g3"),
    Case("grouped_attr_lut", (PUT, jc.ATTR14), jc.C_K32, "attr"),
    Case("grouped_attr_g3_lut", (PUT, E[(1 << 24, -(1 << 23))]), jc.C_K64, "attr_g3"),
    # k_grouped_lds
    Case("lds_hash", (PUT, jc.HASH_WIDE), jc.C_K64, "attr_g3", None, 12),
    Case("lds_lut", (PUT, jc.ATTR25), jc.C_K32, "attr"),
    # k_grouped_global
    Case("global_hash", (PUT, jc.BIG_HASH), jc.C_K64, "attr_g3"),
    Case("global_lut", (PUT, jc.BIG_LUT), jc.C_K32, "attr_g3"),
    # device-built tables: empty payload slots hold INT32_MIN, not -1
    Case("table_raw_wide", (TABLE, "raw_wide"), jc.C_K64, "attr"),
    Case("table_raw_wide_semi", (TABLE, "raw_wide"), jc.C_K64, "semi"),
    Case("table_null_build_keys", (TABLE, "null_keys"), jc.C_K32, "attr"),
    Case("table_dup_semi_keys", (TABLE, "dup_same_attr"), jc.C_K64, "semi"),
    Case("table_deleted_semi", (TABLE, "deleted"), jc.C_K64, "semi"),
] + [
    # NULL fact keys never join; their slot holds a 0 and 0 is a dimension key
    Case("null_%s_%s_%s" % (kn, rn, mode), (PUT, d), kc, mode)
    for kn, kc in (("kn64", jc.C_KN64), ("kn32", jc.C_KN32))
    for rn, d in (("hash", jc.HASH_WIDE), ("lut", E[(204800, -100000)]))
    for mode in ("semi", "attr")
]
assert all(0 in c.src[1].keys for c in INTERPRETED if c.id.startswith("null_"))


# ------------------------------------------------------------------ loading


def load_fact(eng, fx, name):
    t = eng.table_define(name, jc.SCHEMA)
    for bi, (s, e) in enumerate(fx.bounds()):
        part = []
        for c, (_dt, nullable) in enumerate(jc.SCHEMA):
            col = {"data": np.ascontiguousarray(fx.cols[c][s:e])}
            if nullable and not fx.valid[c][s:e].all():
                col["valid"] = fx.valid[c][s:e].astype(np.uint8)
            part.append(col)
        n = e - s
        assert eng.ingest_columns(t, part, n, batch_rows=n, first_bucket=bi) == n
    return t


def build_table(eng, b, name):
    """the build-side column table of jc.Build b, as its `how` says"""
    n = len(b.keys)
    nullable = not all(b.valid)
    np_t = np.int64 if b.key_type == po.T_INT64 else np.int32
    keys = np.array(b.keys, dtype=np_t)
    valid = np.array(b.valid, dtype=np.uint8)
    t = eng.table_define(name, [(b.key_type, nullable), (abi.T_STRING, False)])
    if b.how == "raw":
        kcol = {"data": keys}
        if nullable:
            kcol["valid"] = valid
        assert not b.deleted and not b.patch
        assert eng.ingest_columns(
            t, [kcol, {"data": b"".join(b.attrs),
                       "lens": np.array([len(a) for a in b.attrs], dtype=np.int32)}],
            n, batch_rows=n) == n
        return t
    blobs = [po.encode(b.key_type, po.ENC_UNCOMPRESSED, keys,
                       valid if nullable else None),
             po.encode(po.T_STRING, po.ENC_DICT, b.attrs)]
    stats = mask = deltas = None
    if b.stats is not None:
        stats = po.encode_stats([b.key_type, po.T_STRING], -n if b.patch else n,
                                [b.stats[0], 0], [b.stats[1], 0],
                                null_counts=[0, 0], has_bounds=[1, 0])
    if b.deleted:
        mask = po.encode_delete(b.deleted, n)
    if b.patch:
        pos = np.array(sorted(b.patch), dtype=np.int32)
        newv = np.array([b.patch[int(p)] for p in pos], dtype=np_t)
        deltas = [(se.encode_update_delta(b.key_type, pos, n, newv), None),
                  (None, None)]
    eng.batch_put(t, 1, 0, -n if deltas else n, blobs, stats=stats,
                  delete_mask=mask, deltas=deltas)
    return t


def make_dim(eng, case, tag):
    """(dimension handle, keys, attrs, the dimension set the fact draws)"""
    kind, what = case.src
    d = eng.dim_define("d_" + tag)
    by_attr = case.mode.startswith("attr")
    if kind == PUT:
        attrs = what.attrs(case.nattr)
        eng.dim_put(d, np.array(what.keys, dtype=np.int64),
                    attrs if by_attr else None)
        return d, what.keys, attrs, what
    b = jc.BUILDS[what]
    bt = build_table(eng, b, "b_" + tag)
    eng.dim_from_table(d, bt, key_col=0, attr_col=1 if by_attr else -1)
    keys, attrs = b.effective()
    return d, keys, attrs, jc.BUILD_FACT[what]


def check(eng, t, fx, case, d, keys, attrs):
    exp = jc.reference(fx, case.key_col, keys, attrs, case.mode, case.aggs)
    q = eng.query(abi.make_plan(
        table=t, **jc.plan_args(case.mode, case.key_col, d, case.aggs)))
    rows = q.rows()
    got = {k: v for k, v in rows}
    assert len(rows) == len(got) == len(exp) > 0
    assert got == exp
    return q


# ------------------------------------------------------------------- tests


@pytest.mark.parametrize("case", COMPILED, ids=[c.id for c in COMPILED])
def test_compiled_probe(case, monkeypatch, tmp_path):
    dump = tmp_path / "jit.cu"
    monkeypatch.setenv("SN_JIT_DUMP", str(dump))
    eng = se.Engine(device=0)           # fresh: nothing cached hides the dump
    try:
        d, keys, attrs, factset = make_dim(eng, case, case.id)
        fx = jc.fact(factset, interpreted=False)
        t = load_fact(eng, fx, "f_" + case.id)
        q = check(eng, t, fx, case, d, keys, attrs)
        assert q.used_jit()
        q.close()
        src = dump.read_text()
        for probe, mark in MARKS.items():
            assert (mark in src) == (probe == case.probe), (probe, case.probe)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def shared():
    eng = se.Engine(device=0)
    tables = {}

    def fact_table(factset):
        if factset.name not in tables:
            fx = jc.fact(factset, interpreted=True)
            tables[factset.name] = (load_fact(eng, fx, "fi_" + factset.name), fx)
        return tables[factset.name]
    yield eng, fact_table
    eng.close()


@pytest.mark.parametrize("case", INTERPRETED, ids=[c.id for c in INTERPRETED])
def test_interpreted_probe(case, shared):
    eng, fact_table = shared
    d, keys, attrs, factset = make_dim(eng, case, case.id)
    t, fx = fact_table(factset)
    q = check(eng, t, fx, case, d, keys, attrs)
    assert not q.used_jit()
    q.close()


def test_int64_min_is_not_a_dimension_key(shared):
    """INT64_MIN marks an empty slot of the device table: sn_dim_put refuses
    it, as sn_dim_from_table does"""
    eng, fact_table = shared
    t, _fx = fact_table(jc.EXTREME)
    d = eng.dim_define("d_int64_min")
    with pytest.raises(se.EngineError):
        eng.dim_put(d, np.array([1, jc.I64_MIN, 3], dtype=np.int64))
        eng.query(abi.make_plan(
            table=t, **jc.plan_args("semi", jc.C_K64, d))).rows()
    # and the refused put left nothing behind
    eng.dim_put(d, np.array([1, 3], dtype=np.int64))
