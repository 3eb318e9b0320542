#!/usr/bin/env python3
"""bench.py — the driver-facing benchmark of the MI355X columnar engine.

Workload (BASELINE.json): the hot path scan -> filter -> aggregate on TPC-H
lineitem.  A "step" is one full pass of the hot path over the resident
synthetic table (all column batches, one kernel launch).  Default workload at
N=1 is `tpch_q6_lineitem_sf100` — the SF=100 configuration BASELINE.json's
metric is quoted on (600M rows x 28 B = 17 GB, well inside one GPU's 288 GB
HBM; configs[0] is the reference's CPU-only case, configs[1] the smaller
SF=10 warmer, both selectable via --workload).  Inputs are generated once
(seeded, synthetic — no network) and resident in HBM before the timed region.

Multi-GPU (--gpus N, launched by torch.distributed.run, one rank per GPU over
RCCL): column batches shard by bucket across ranks (weak scaling — per-GPU
rows fixed); the keyless Q6 partial state is exchanged with an RCCL all_reduce
over xGMI, mirroring the reference's partial->final aggregation exchange.

Output: ONE JSON line from rank 0 per the driver contract, including
`ms_per_step` (wall milliseconds per timed step; --steps sets their number)
and `roofline` (achieved HBM GB/s of the scan kernel from the HIP events the
timed steps already record on its launch stream, vs the 8 TB/s chip peak).

A plain run sets up, warms up, times the steps and prints the line.  --full
adds `cpu_baseline` (the CPU oracle — a faithful restatement of the
reference's WholeStageCodegen loop — timed on the host cores over a bounded
sample; the reference itself is JVM-only and cannot run here: BASELINE.md);
without --full that field is null.  --dump-outputs DIR writes the result
rows of the last timed step as DIR/values.npy, plus DIR/keys.npy when the
result is grouped (see dump_outputs); inputs are seeded, so equal arguments give equal inputs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

from snappydata_amd import abi, engine as se  # noqa: E402

HBM_PEAK_GBPS = 8000.0   # MI355X spec peak (MI355X_MICROARCH.md)


def days(y, m, d):
    import datetime
    return (datetime.date(y, m, d) - datetime.date(1970, 1, 1)).days


LINEITEM_SCHEMA = [(abi.T_DOUBLE, False)] * 4 + [(abi.T_STRING, False)] * 2 + \
    [(abi.T_INT32, False)]
COL_QTY, COL_EP, COL_DISC, COL_TAX, COL_RF, COL_LS, COL_SHIP = range(7)


def q6_plan(table):
    return abi.make_plan(
        table=table,
        preds=[dict(col=COL_SHIP, lo=days(1994, 1, 1), hi=days(1995, 1, 1),
                    hi_strict=True),
               dict(col=COL_DISC, is_double=True, lo=0.05, hi=0.07),
               dict(col=COL_QTY, is_double=True, hi=24.0, hi_strict=True)],
        aggs=[("sum", [(COL_EP, 0.0, 1.0), (COL_DISC, 0.0, 1.0)])])


def q1_plan(table):
    cutoff = days(1997, 12, 31) - 90
    return abi.make_plan(
        table=table,
        preds=[dict(col=COL_SHIP, hi=cutoff)],
        group_cols=[COL_RF, COL_LS],
        aggs=[("sum", [(COL_QTY, 0.0, 1.0)]),
              ("sum", [(COL_EP, 0.0, 1.0)]),
              ("sum", [(COL_EP, 0.0, 1.0), (COL_DISC, 1.0, -1.0)]),
              ("sum", [(COL_EP, 0.0, 1.0), (COL_DISC, 1.0, -1.0),
                       (COL_TAX, 1.0, 1.0)]),
              ("avg", [(COL_QTY, 0.0, 1.0)]),
              ("avg", [(COL_EP, 0.0, 1.0)]),
              ("avg", [(COL_DISC, 0.0, 1.0)]),
              ("count", [])])


WORKLOADS = {
    # name: (plan fn, rows per GPU, algorithmic bytes per row read by the scan)
    "tpch_q6_lineitem_sf10": (q6_plan, 60_000_000, 28),   # ship4+qty8+ep8+disc8
    "tpch_q6_lineitem_sf100": (q6_plan, 600_000_000, 28),
    "tpch_q1_lineitem_sf100": (q1_plan, 600_000_000, 40),  # +tax8+2x2dict, ship4
    "tpch_q1_lineitem_sf10": (q1_plan, 60_000_000, 40),
    # BASELINE config 5: Q6 scan with ~2% of rows update-patched and ~1%
    # deleted (ColumnDeltaDecoder/delete-mask merge during the scan)
    "tpch_q6_mut_sf10": (q6_plan, 60_000_000, 28),
    # BASELINE config 4: star schema — column fact (suppkey, extendedprice)
    # joined to a broadcast row-store dimension, group by dim attribute
    "star_join_sf10": (None, 60_000_000, 12),
    # BASELINE config 1 (the reference's CPU-runnable case): 10M rows
    # (int32, f64), SELECT SUM(d), COUNT(*) WHERE i > median
    "config1_sum_where": (None, 10_000_000, 12),
    # sparse-key open-address hash aggregate (the SHAMap analogue): 60M rows,
    # ~1M distinct int64 keys — no dense slot structure, pure hash probe
    "sparse_group_sf10": (None, 60_000_000, 16),
}

# roofline bound per workload: every scan shape is HBM-bound EXCEPT the
# star join, whose PMC wave-cycle profile shows probe issue-stall, not HBM
# saturation (profiles/star_join_sf10_wavecycles_*.csv) — labeling it
# "hbm" would overstate headroom against the 8 TB/s peak
WORKLOAD_BOUND = {"star_join_sf10": "latency"}

# pipeline workloads whose dominant-kernel algorithmic bytes exceed the
# input bytes: the radix two-pass hash aggregate streams input (16) +
# record write (16) + record read (16) per row; PMC traffic additionally
# shows the 16 B-record scatter's sector amplification
ALG_PIPELINE_BYTES = {"sparse_group_sf10": 48}


def build_config1(eng, t, total_rows, seed, batch_rows=600_000):
    rng = np.random.default_rng(seed)
    i32 = rng.integers(0, 10**6, total_rows).astype(np.int32)
    d = rng.random(total_rows)
    eng.ingest_columns(t, [{"data": i32}, {"data": d}], total_rows,
                       batch_rows=batch_rows)
    k = int(np.median(i32))
    return abi.make_plan(table=t, preds=[dict(col=0, lo=k, lo_strict=True)],
                         aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])])


def build_star_join(eng, t, total_rows, seed, batch_rows=2_000_000,
                    dist=None, rank=0, device="cpu"):
    """Fact (suppkey int32, extendedprice f64) + dimension covering 40% of a
    100K keyspace with 8 nation attributes (dimension << HashJoinSize).
    At N>1 rank 0 generates the dimension and BROADCASTS it over RCCL into
    every rank's HBM — the reference's replicated row-store region handed
    to each executor once (host region get() -> broadcast)."""
    rng = np.random.default_rng(seed)
    keyspace = 100_000
    for start in range(0, total_rows, batch_rows):
        n = min(batch_rows, total_rows - start)
        keys = rng.integers(0, keyspace, n).astype(np.int32)
        ep = rng.random(n) * 1e5
        eng.ingest_columns(t, [{"data": keys}, {"data": ep}], n,
                           batch_rows=batch_rows,
                           first_bucket=start // batch_rows)
    dim = eng.dim_define("supplier")
    ndim = keyspace * 2 // 5
    if dist is None:
        dk = np.sort(rng.choice(keyspace, size=ndim,
                                replace=False)).astype(np.int64)
    else:
        import torch
        if rank == 0:
            dk_np = np.sort(rng.choice(keyspace, size=ndim,
                                       replace=False)).astype(np.int64)
            dk_t = torch.from_numpy(dk_np).to(device)
        else:
            dk_t = torch.empty(ndim, dtype=torch.int64, device=device)
        dist.broadcast(dk_t, src=0)
        dk = dk_t.cpu().numpy()
    attrs = [b"NATION_%d" % (int(k) % 8) for k in dk]
    eng.dim_put(dim, dk, attrs)
    plan = abi.make_plan(table=t,
                         aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])],
                         join=dict(dim=dim, fact_col=0, group=True))
    return plan


def build_sparse_group(eng, t, total_rows, seed, batch_rows=600_000):
    """Sparse-key hash-aggregate workload: ~1M distinct int64 keys scattered
    over the full 64-bit space — no stats-derived dense span, so every row
    probes the open-address table (the SHAMap-analogue path)."""
    rng = np.random.default_rng(seed)
    ndistinct = 1_000_000
    universe = rng.integers(-2**62, 2**62, ndistinct).astype(np.int64)
    for start in range(0, total_rows, batch_rows):
        n = min(batch_rows, total_rows - start)
        keys = universe[rng.integers(0, ndistinct, n)]
        w = rng.random(n)
        eng.ingest_columns(t, [{"data": keys}, {"data": w}], n,
                           batch_rows=batch_rows,
                           first_bucket=start // batch_rows)
    return abi.make_plan(table=t, group_cols=[0],
                         aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])])


def build_mutable_lineitem(eng, t, total_rows, seed, batch_rows=600_000):
    """Config-5 table: product-encoded batches carrying update deltas on
    l_discount (~2% of rows) and delete masks (~1%)."""
    rng = np.random.default_rng(seed + 1)
    bi = 0
    for start in range(0, total_rows, batch_rows):
        n = min(batch_rows, total_rows - start)
        d = se.gen_lineitem_arrays(start, n, seed)
        cols = [se.encode_column(abi.T_DOUBLE, d["qty"]),
                se.encode_column(abi.T_DOUBLE, d["ep"]),
                se.encode_column(abi.T_DOUBLE, d["disc"]),
                se.encode_column(abi.T_DOUBLE, d["tax"]),
                se.encode_column(abi.T_STRING, b"".join(d["rf"]),
                                 lens=np.ones(n, dtype=np.int32)),
                se.encode_column(abi.T_STRING, b"".join(d["ls"]),
                                 lens=np.ones(n, dtype=np.int32)),
                se.encode_column(abi.T_INT32, d["ship"])]
        upd = np.unique(rng.integers(0, n, max(1, n // 50))).astype(np.int32)
        d1 = se.encode_update_delta(abi.T_DOUBLE, upd, n,
                                    rng.integers(0, 11, len(upd)) / 100.0)
        deltas = [(None, None), (None, None), (d1, None), (None, None),
                  (None, None), (None, None), (None, None)]
        dels = np.unique(rng.integers(0, n, max(1, n // 100))).astype(np.int32)
        dmask = se.encode_delete_mask(dels, n)
        eng.batch_put(t, bi, bi, -n, cols, delete_mask=dmask, deltas=deltas)
        bi += 1


def _pmc_traffic(workload, resident_rows):
    try:
        cal = json.load(open(os.path.join(REPO, "profiles", "traffic.json")))
        return round(cal[workload]["bytes_per_row"] * resident_rows)
    except Exception:
        return None


def cpu_baseline_leg(workload, seed, target_seconds=10.0, sample_rows=None):
    """Time the CPU oracle (reference-loop restatement, OpenMP over all host
    cores) on a bounded sample of the same workload.  Returns the dict for
    the JSON line."""
    from oracle import pyoracle as po
    from tests import tpch_util as tu

    sample_rows = sample_rows or 24_000_000
    batch_rows = 300_000        # >= one batch per thread, or cores idle
    cores = os.cpu_count()
    run_fn = None
    if workload == "sparse_group_sf10":
        # generic per-row loop + open hash table (the oracle's SHAMap
        # restatement); result set ~1M groups -> flat export
        sample_rows = min(sample_rows, 2_400_000)
        rng = np.random.default_rng(seed)
        universe = rng.integers(-2**62, 2**62, 1_000_000).astype(np.int64)
        keys = universe[rng.integers(0, 1_000_000, sample_rows)]
        w = rng.random(sample_rows)
        t = po.OracleTable([po.T_INT64, po.T_DOUBLE])
        for st in range(0, sample_rows, batch_rows):
            en = min(sample_rows, st + batch_rows)
            t.add_batch(en - st,
                        [po.encode(po.T_INT64, po.ENC_UNCOMPRESSED, keys[st:en]),
                         po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, w[st:en])])
        plan = po.make_plan(group_cols=[0],
                            aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])])
        nthreads = min(cores, sample_rows // batch_rows)
        run_fn = lambda: t.query_groups(plan, nthreads=nthreads, cap=1 << 21)  # noqa: E731
    elif workload == "star_join_sf10":
        # generic oracle loop (the join keeps the per-row path): smaller
        # sample so the calibration pass stays bounded
        sample_rows = min(sample_rows, 2_400_000)
        rng = np.random.default_rng(seed)
        keyspace = 100_000
        keys = rng.integers(0, keyspace, sample_rows).astype(np.int32)
        ep = rng.random(sample_rows) * 1e5
        t = po.OracleTable([po.T_INT32, po.T_DOUBLE])
        for st in range(0, sample_rows, batch_rows):
            en = min(sample_rows, st + batch_rows)
            t.add_batch(en - st,
                        [po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, keys[st:en]),
                         po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, ep[st:en])])
        dk = np.sort(rng.choice(keyspace, size=keyspace * 2 // 5,
                                replace=False)).astype(np.int64)
        t.set_dim(dk, [b"NATION_%d" % (int(k) % 8) for k in dk])
        plan = po.make_plan(aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])],
                            join=dict(dim=0, fact_col=0, group=True))
    elif workload == "config1_sum_where":
        rng = np.random.default_rng(seed)
        i32 = rng.integers(0, 10**6, sample_rows).astype(np.int32)
        dv = rng.random(sample_rows)
        t = po.OracleTable([po.T_INT32, po.T_DOUBLE])
        for st in range(0, sample_rows, batch_rows):
            en = min(sample_rows, st + batch_rows)
            t.add_batch(en - st,
                        [po.encode(po.T_INT32, po.ENC_UNCOMPRESSED, i32[st:en]),
                         po.encode(po.T_DOUBLE, po.ENC_UNCOMPRESSED, dv[st:en])])
        plan = po.make_plan(preds=[dict(col=0, lo=int(np.median(i32)),
                                        lo_strict=True)],
                            aggs=[("sum", [(1, 0.0, 1.0)]), ("count", [])])
    else:
        d = se.gen_lineitem_arrays(0, sample_rows, seed)
        t = po.OracleTable(tu.LINEITEM_DTYPES)
        for num_rows, cols, stats in tu.encode_lineitem_batches(d, batch_rows):
            t.add_batch(num_rows, cols, stats=stats)
        plan = tu.q6_plan() if "q6" in workload else tu.q1_plan()
    # threads beyond the batch count only add fork/merge overhead
    nthreads = min(cores, sample_rows // batch_rows)
    if run_fn is None:
        run_fn = lambda: t.query(plan, nthreads=nthreads)  # noqa: E731
    # one calibration pass, then enough reps for ~target_seconds
    t0 = time.perf_counter()
    run_fn()
    t1 = time.perf_counter()
    reps = max(1, int(target_seconds / max(1e-3, t1 - t0)))
    t0 = time.perf_counter()
    for _ in range(reps):
        run_fn()
    dt = time.perf_counter() - t0
    return {
        "value": sample_rows * reps / dt,
        "unit": "rows/s",
        "cores": nthreads,
        "kind": "port",
        "sample": f"{sample_rows} rows x {reps} passes ({dt:.1f}s) of the same "
                  f"synthetic workload through the CPU oracle (OpenMP, "
                  f"{nthreads} of {cores} host threads"
                  + (", generic per-row loop — the oracle has no "
                     "codegen-shaped fast path for joins"
                     if workload == "star_join_sf10" else "")
                  + "; no JVM available for the reference itself)",
    }


DUMP_BUDGET_BYTES = 64 << 20
DUMP_KEY_BYTES = 24          # longest key text: a decimal int64 is 20 chars
DUMP_KEY_WORDS = DUMP_KEY_BYTES // 6


def dump_outputs(dirname, rows, seed):
    """Write the result rows a caller of the timed path receives — a list of
    (group-key tuple, aggregate values) — as float64 arrays:
      values.npy  (nrows, naggs)   NULL aggregates as NaN
      keys.npy    (nrows, ngroup, 4) each key's text, zero-padded to 24
                  bytes and packed 6 bytes (big-endian) per float64 so it is
                  exact; NULL keys as NaN; written only for grouped
                  results (a keyless result such as Q6 has no keys)
    Rows are sorted by key so two builds compare row for row whatever order
    the hash aggregate emitted them in.  A result set over the 64 MB budget
    is cut to a fixed, seeded sample of the sorted rows."""
    rows = sorted(rows, key=lambda r: tuple((k is None, k or "")
                                            for k in r[0]))
    ngroup = len(rows[0][0]) if rows else 0
    naggs = len(rows[0][1]) if rows else 0
    row_bytes = 8 * (naggs + ngroup * DUMP_KEY_WORDS)
    cap = DUMP_BUDGET_BYTES // max(1, row_bytes)
    if len(rows) > cap:
        pick = np.sort(np.random.default_rng(seed).choice(
            len(rows), size=cap, replace=False))
        rows = [rows[i] for i in pick]
    values = np.array([[np.nan if v is None else v for v in vals]
                       for _, vals in rows], dtype=np.float64)
    values = values.reshape(len(rows), naggs)
    keys = np.full((len(rows), ngroup, DUMP_KEY_WORDS), np.nan)
    for r, (ks, _) in enumerate(rows):
        for g, k in enumerate(ks):
            if k is None:
                continue
            raw = k.encode()[:DUMP_KEY_BYTES].ljust(DUMP_KEY_BYTES, b"\0")
            keys[r, g] = [int.from_bytes(raw[i:i + 6], "big")
                          for i in range(0, DUMP_KEY_BYTES, 6)]
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "values.npy"), values)
    keys_path = os.path.join(dirname, "keys.npy")
    if ngroup:
        np.save(keys_path, keys)
    elif os.path.exists(keys_path):
        os.remove(keys_path)      # a keyless result has no key array


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20,
                    help="timed steps (at least 1)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="tpch_q6_lineitem_sf100",
                    choices=sorted(WORKLOADS))
    ap.add_argument("--rows", type=int, default=0,
                    help="override rows per GPU")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--full", action="store_true",
                    help="also run the legs the headline figure does not "
                         "need (the CPU-oracle baseline)")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU-oracle baseline leg")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's result rows to "
                         "DIR/values.npy, and DIR/keys.npy when grouped "
                         "(float64)")
    ap.add_argument("--no-a2a", action="store_true",
                    help="use all_gather instead of the key-sharded "
                         "all-to-all for the grouped exchange (N>1)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n_gpus = max(world, args.gpus if world == 1 else world)

    dist = None
    torch = None
    if world > 1:
        import torch as _torch
        import torch.distributed as _dist
        torch = _torch
        torch.cuda.set_device(local_rank)
        _dist.init_process_group("nccl")
        dist = _dist

    plan_fn, default_rows, bytes_per_row = WORKLOADS[args.workload]
    rows_per_gpu = args.rows or default_rows
    total_rows = rows_per_gpu * n_gpus

    eng = se.Engine(device=local_rank, shard_rank=rank, shard_count=world,
                    n_buckets=max(128, world * 16))
    t_ingest0 = time.perf_counter()
    if args.workload == "star_join_sf10":
        t = eng.table_define("fact", [(abi.T_INT32, False), (abi.T_DOUBLE, False)])
        plan = build_star_join(eng, t, total_rows, args.seed, dist=dist,
                               rank=rank,
                               device=f"cuda:{local_rank}" if dist else "cpu")
    elif args.workload == "config1_sum_where":
        t = eng.table_define("c1", [(abi.T_INT32, False), (abi.T_DOUBLE, False)])
        plan = build_config1(eng, t, total_rows, args.seed)
    elif args.workload == "sparse_group_sf10":
        t = eng.table_define("sg", [(abi.T_INT64, False), (abi.T_DOUBLE, False)])
        plan = build_sparse_group(eng, t, total_rows, args.seed)
    else:
        t = eng.table_define("lineitem", LINEITEM_SCHEMA)
        if args.workload == "tpch_q6_mut_sf10":
            build_mutable_lineitem(eng, t, total_rows, args.seed)
        else:
            eng.datagen_lineitem(t, total_rows, seed=args.seed, batch_rows=600_000)
        plan = plan_fn(t)
    resident = eng.num_rows(t)
    # PCIe-inclusive producer rate (generate + encode + stats + put + H2D),
    # outside the timed region — the config-5 ingest observability
    ingest_s = time.perf_counter() - t_ingest0
    grouped = plan.ngroup > 0 or plan.join_mode == 1 and plan.join_dim >= 0

    exchange_buf = None

    jit_used = {"v": False}
    # workloads whose result set is huge (~1M groups): materializing the
    # row list per step is host-side work the reference also does outside
    # its operator loop (result iteration) — count groups once, untimed
    heavy_result = args.workload == "sparse_group_sf10"

    kept = {}

    def step(keep=False):
        q = eng.query(plan)
        q.wait()
        km = q.kernel_ms()
        jit_used["v"] = q.used_jit()
        if dist is not None:
            if not grouped:
                # RCCL all_reduce of the fixed-width keyless partial block
                nonlocal exchange_buf
                n = q.partial_bytes()
                assert n % 8 == 0
                if exchange_buf is None:
                    exchange_buf = torch.zeros(n // 8, dtype=torch.float64,
                                               device=f"cuda:{local_rank}")
                q.partials_into_device(exchange_buf.data_ptr())
                dist.all_reduce(exchange_buf)
                merged = exchange_buf.cpu().numpy().view(np.uint8)
                q.merge_host(np.ascontiguousarray(merged), n, 1)
            elif not args.no_a2a:
                # key-sharded RCCL all-to-all (the default
                # grouped exchange — BASELINE's 8-GPU Q1 shape): rank r keeps
                # only groups hashing to shard r; each rank merges the
                # world blocks it received and holds its final key subset
                # (the reference's hash-partitioned partial->final shuffle).
                # Block capacity is negotiated per step (allreduce-MAX of
                # local group counts) so overflow group-bys — the north-star
                # "hash table overflows one GPU" demo — exchange cleanly.
                cap_t = torch.tensor([max(1024, q.num_groups())],
                                     dtype=torch.int64,
                                     device=f"cuda:{local_rank}")
                dist.all_reduce(cap_t, op=dist.ReduceOp.MAX)
                cap = int(cap_t.item())
                n = q.partial_bytes(cap)
                send = torch.from_numpy(
                    q.partials_sharded(world, cap).reshape(-1)).to(
                        f"cuda:{local_rank}")
                recv = torch.empty_like(send)
                dist.all_to_all_single(recv, send)
                blocks = recv.cpu().numpy()
                q.merge_host(np.ascontiguousarray(blocks), n, world)
            else:
                # RCCL all_gather of self-describing grouped partial blocks
                cap_t = torch.tensor([max(1024, q.num_groups())],
                                     dtype=torch.int64,
                                     device=f"cuda:{local_rank}")
                dist.all_reduce(cap_t, op=dist.ReduceOp.MAX)
                cap = int(cap_t.item())
                n = q.partial_bytes(cap)
                local = torch.from_numpy(q.partials_host(cap)).to(
                    f"cuda:{local_rank}")
                gathered = torch.zeros(world * n, dtype=torch.uint8,
                                       device=f"cuda:{local_rank}")
                dist.all_gather_into_tensor(gathered, local)
                blocks = gathered.cpu().numpy()
                q.merge_host(np.ascontiguousarray(blocks), n, world)
        rows = q.rows() if not heavy_result else None
        if keep:
            kept["q"] = q     # --dump-outputs reads its rows after the timer
        else:
            q.close()
        return rows, km

    n_result_rows = {"v": 0}

    def barrier_sync():
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    # warmup
    result = None
    for _ in range(max(1, args.warmup)):
        result, _ = step()
    if heavy_result:
        qc = eng.query(plan)
        qc.wait()
        n_result_rows["v"] = qc.num_groups()
        qc.close()
    elif result:
        n_result_rows["v"] = len(result)

    barrier_sync()
    kms = []
    t0 = time.perf_counter()
    keep_last = heavy_result and args.dump_outputs is not None
    for i in range(args.steps):
        result, km = step(keep_last and i == args.steps - 1)
        if km > 0:
            kms.append(km)
    barrier_sync()
    elapsed = time.perf_counter() - t0

    if dist is not None:
        e_t = torch.tensor([elapsed], dtype=torch.float64,
                           device=f"cuda:{local_rank}")
        dist.all_reduce(e_t, op=dist.ReduceOp.MAX)
        elapsed = float(e_t.cpu())

    if "q" in kept:
        result = kept["q"].rows()
        kept.pop("q").close()
    if args.dump_outputs is not None and rank == 0:
        dump_outputs(args.dump_outputs, result, args.seed)

    ms_per_step = elapsed * 1000.0 / args.steps
    value = total_rows * args.steps / elapsed

    if rank == 0:
        # roofline: dominant kernel = the single fused scan kernel.
        # achieved = algorithmic bytes per launch / avg kernel time.
        roofline = None
        if kms:
            avg_ms = float(np.mean(kms))
            alg_bytes = resident * ALG_PIPELINE_BYTES.get(
                args.workload, bytes_per_row)        # this rank's launch
            achieved = alg_bytes / (avg_ms / 1000.0) / 1e9
            roofline = {
                "bound": WORKLOAD_BOUND.get(args.workload, "hbm"),
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBPS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBPS, 4),
                # PMC-measured HBM bytes/launch (rocprofv3 FETCH_SIZE x2 +
                # WRITE_SIZE, collected per profiles/README.md) scaled to
                # this run's resident rows; null when unmeasured
                "traffic": _pmc_traffic(args.workload, resident),
                "kernel_ms": round(avg_ms, 4),
            }
        cpu_baseline = None
        if args.full and world == 1 and not args.no_cpu_baseline and (
                "lineitem" in args.workload or "mut" in args.workload
                or args.workload in ("config1_sum_where", "star_join_sf10",
                                     "sparse_group_sf10")):
            cpu_baseline = cpu_baseline_leg(args.workload, args.seed)

        line = {
            "metric": "rows/sec scan+filter+agg (TPC-H lineitem)",
            "value": round(value, 1),
            "unit": "rows/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,     # no absolute published numbers
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": args.workload,
                "rows_per_gpu": rows_per_gpu,
                "total_rows": total_rows,
                "bytes_per_row": bytes_per_row,
                "batch_rows": 600_000,
                "parallelism": f"bucket-dp{n_gpus}",
                "result_rows": n_result_rows["v"],
                "jit": jit_used["v"],   # query-compiled (hipRTC) kernel ran
                "ingest_s": round(ingest_s, 2),
                "ingest_rows_per_s": round(resident / max(1e-9, ingest_s)),
            },
            "roofline": roofline,
            "cpu_baseline": cpu_baseline,
        }
        print(json.dumps(line))

    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
