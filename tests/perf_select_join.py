"""Perf driver of the join row scans (not a pytest).  Run on a GPU box:

    python tests/perf_select_join.py [--legs join,plain,ordered] [--tag NAME]

join     bench.build_star_join's data (star_join_sf10: 60M rows, suppkey int32
         + extendedprice f64, 40K-key dimension, 8 attributes): configurations
         (a)-(g) of DESIGN.md 3f.  The table has no date column, so (g)'s
         range predicate is on extendedprice and keeps 3 % of the rows.
plain    configuration (a) alone: a plain select, key and price projected.
ordered  the ordered configuration of profiles/order_scan_sf10_r01.txt:
         lineitem 60M rows, Q6 predicates, ORDER BY l_extendedprice DESC
         LIMIT 100, key + ROWID projected.

`plain` and `ordered` use nothing the join scan added, so this file also runs
from a checkout without it: the no-slowdown comparison.  Each configuration:
3 warm-up submits, the median kernel_ms of 11 timed ones, two alternating
rounds; mark / offsets / gather come from sn_rows_kernel_ms."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import bench  # noqa: E402
from snappydata_amd import abi, engine as se  # noqa: E402
from tests import tpch_util as tu  # noqa: E402

WARM, TIMED, ROUNDS = 3, 11, 2


def timed(name, tag, rnd, submit):
    for _ in range(WARM):
        q = submit()
        q.wait()
        q.close()
    ms, parts, info = [], [], ""
    for _ in range(TIMED):
        q = submit()
        q.wait()
        ms.append(q.kernel_ms())
        if hasattr(q, "kernel_ms_parts"):
            parts.append(q.kernel_ms_parts())
            info = f" rows={q.count()} rows_passed={q.rows_passed()}"
        q.close()
    line = (f"{name} tag={tag} round={rnd}{info} kernel_ms={np.median(ms):.4f} "
            f"min={min(ms):.4f} max={max(ms):.4f}")
    if parts:
        p = np.median(np.array(parts), axis=0)
        line += f" mark={p[0]:.4f} offsets={p[1]:.4f} gather={p[2]:.4f}"
    print(line, flush=True)


def star(eng):
    t = eng.table_define("star_fact", [(abi.T_INT32, False),
                                       (abi.T_DOUBLE, False)])
    agg_plan = bench.build_star_join(eng, t, 60_000_000, 42)
    return t, agg_plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="join,plain,ordered")
    ap.add_argument("--tag", default="this")
    args = ap.parse_args()
    legs = args.legs.split(",")
    eng = se.Engine(device=0)
    configs = []
    if "join" in legs or "plain" in legs:
        t, agg_plan = star(eng)
        dim = agg_plan.join_dim
        plain = abi.make_plan(table=t)
        configs.append(("a_plain_select",
                        lambda: eng.select(plain, [0, 1])))
    if "join" in legs:
        jp = abi.make_plan(table=t, join=dict(dim=dim, fact_col=0))
        few = dict(col=1, is_double=True, lo=0.0, hi=3000.0, hi_strict=True)
        jp_few = abi.make_plan(table=t, preds=[few],
                               join=dict(dim=dim, fact_col=0))
        A = abi.PROJ_DIM_ATTR
        configs += [
            ("b_inner", lambda: eng.select(jp, [0, 1],
                                           join_type=abi.RJOIN_INNER)),
            ("c_inner_attr", lambda: eng.select(jp, [0, 1, A],
                                                join_type=abi.RJOIN_INNER)),
            ("d_left_outer_attr", lambda: eng.select(
                jp, [0, 1, A], join_type=abi.RJOIN_LEFT_OUTER)),
            ("e_left_anti", lambda: eng.select(
                jp, [0, 1], join_type=abi.RJOIN_LEFT_ANTI)),
            ("f_aggregate_star_join", lambda: eng.query(agg_plan)),
            ("g_inner_attr_3pct", lambda: eng.select(
                jp_few, [0, 1, A], join_type=abi.RJOIN_INNER)),
        ]
    if "ordered" in legs:
        li = eng.table_define("li", [(abi.T_DOUBLE, False)] * 4 +
                              [(abi.T_STRING, False)] * 2 +
                              [(abi.T_INT32, False)])
        eng.datagen_lineitem(li, 60_000_000, seed=42, batch_rows=600_000)
        q6 = abi.make_plan(table=li, preds=[
            dict(col=tu.COL_SHIP, lo=tu.days(1994, 1, 1),
                 hi=tu.days(1995, 1, 1), hi_strict=True),
            dict(col=tu.COL_DISC, is_double=True, lo=0.05, hi=0.07),
            dict(col=tu.COL_QTY, is_double=True, hi=24.0, hi_strict=True)])
        configs.append(("ordered_q6_extendedprice_desc_100", lambda: eng.select(
            q6, [tu.COL_EP, abi.PROJ_ROWID], limit=100, order_by=tu.COL_EP,
            descending=True)))
    for rnd in range(1, ROUNDS + 1):
        for name, submit in configs:
            timed(name, args.tag, rnd, submit)
    eng.close()


if __name__ == "__main__":
    main()
