"""The fused bucket matcher's by-value arguments and one-trip block start (chain_fused_k, SOP build): the shapes at
which the changed code can go wrong, each bit-exact against the oracle in rows and delivery order, stats().fused == 1
after every flush. Runs on an MI355X only (-m gpu).

What each group pins:
  short segments   blocks with fewer staged rows than a wave (the clamped row loads) and a bucket whose last segment
                   is short (to_end)
  staging edges    one bucket of exactly FU_ROWS = 2048 rows, one more, and own rows + halo + 1 (1536 + 512 + 1), with
                   700 keys known so the rows of several local keys are regrouped in LDS
  u32 ts offsets   a flush whose timestamps span more than 2^31 ms (less than 2^32): the staged offsets are differences
                   of the view's u32 offsets, the block's 64-bit base feeds out_ts, the carry records cross a gap
  kinds / operators  >, >=, <, <= with e2 on either side, on a double (NaN rows), a long and an int scan column: the
                   8- and 4-byte staging loads and the host's operator folding; e1 filters in the scan's own kind, on
                   another column and absent; a select outside the two-column fast path
  other builds     the builds that share the kernel's source: one-key (C1), arrival-order columns (SDG_FU_OCOLS), the
                   run-time operator build (SDG_FU_NO_SOP, read once per process: a child process) and a constant scan
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import siddhi_amd as sa
from siddhi_amd import workloads as w
from test_gpu_parity import oracle_c_rows

pytestmark = pytest.mark.gpu

HEAD = "@app:playback " + w.STOCK_STREAM + " partition with (symbol of StockStream) begin @info(name = 'query1') from "
TAIL = " insert into M; end;"
SEL2 = " select e1.id as e1id, e2.id as e2id"


def app_of(pattern, select=SEL2):
    return HEAD + pattern + select + TAIL


def product_rows(app, cols, syms, bounds):
    """the product over explicit flush bounds: (ts, every output value) per record, fused == 1 after every flush"""
    rt = sa.SiddhiAppRuntime(app)
    try:
        h = rt.getInputHandler("StockStream")
        ids = np.array([rt.intern(s) for s in syms], dtype=np.uint32)
        rows = []
        for s, e in bounds:
            h.send_columns(cols["ts"][s:e], [cols["id"][s:e], ids[cols["key"][s:e]], cols["price"][s:e],
                                             cols["volume"][s:e]])
            rt.flush(deliver=False)
            assert rt.stats().fused == 1
            types, ts, vals, nulls = rt.raw_outputs(0)
            rows += [(ts[i], tuple(v[i] for v in vals)) for i in range(len(ts))]
        return rows
    finally:
        rt.shutdown()


def even_bounds(n, batches):
    b = np.linspace(0, n, batches + 1).astype(int)
    return [(int(b[i]), int(b[i + 1])) for i in range(batches)]


def check(app, cols, syms, bounds, least):
    ref = oracle_c_rows(app, cols, syms)
    assert len(ref) >= least
    assert product_rows(app, cols, syms, bounds) == ref


# ---- 1. short segments ---------------------------------------------------------------------------------------
def short_cols(case):
    if case == "n37":  # every bucket's only block stages fewer rows than one wave
        return w.c2_columns(37, keys=3, per_ms=1)
    if case == "n1573":
        return w.c2_columns(1536 + 37, keys=3, per_ms=3)
    # one key with exactly own rows + 37: a full segment, then a short last one that reaches the bucket's end
    cols = w.c2_columns(1536 + 37 + 40, keys=3, per_ms=3)
    key = np.zeros(len(cols["ts"]), np.int64)
    key[::40][:20] = 1
    key[7::40][:20] = 2
    cols["key"] = key
    assert int((key == 0).sum()) == 1536 + 37
    return cols


@pytest.mark.parametrize("case", ["n37", "n1573", "key1573"])
def test_short_segments(case, oracle_built):
    cols = short_cols(case)
    check(w.C2_APP, cols, w.symbols(3), [(0, len(cols["ts"]))], 1 if case == "n37" else 101)


# ---- 2. staging edges ----------------------------------------------------------------------------------------
EDGE_KEYS = 700
EDGE_CASES = {"n2048": [(0, 2048)], "n2049": [(0, 2049)], "n1536_512_1": [(0, 1536), (1536, 2048), (2048, 2049)],
              "n3585": [(0, 2048 + 1536 + 1)]}


def edge_cols(n):
    """700 keys known, the events on three of them that share a bucket (ids congruent mod 256): one bucket's rows of
    three local keys"""
    cols = w.c2_columns(n, keys=3, per_ms=3)
    cols["key"] = np.array([5, 5 + 256, 5 + 512], np.int64)[cols["key"]]
    return cols


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_staging_edges(case, oracle_built):
    bounds = EDGE_CASES[case]
    check(w.C2_APP, edge_cols(bounds[-1][1]), w.symbols(EDGE_KEYS), bounds, 101)


# ---- 3. u32 timestamp offsets --------------------------------------------------------------------------------
TS_BOUNDS = [(0, 1500), (1500, 3250), (3250, 5000)]


def gap_cols():
    """ten bursts of 500 events in 1 s each, 2^30 + 10^7 ms apart: the first flush ends with a burst (its pending
    partials are carried across a gap), the others span three gaps = more than 2^31 ms, less than 2^32"""
    n, burst, gap = 5000, 500, (1 << 30) + 10_000_000
    cols = w.c2_columns(n, keys=300, per_ms=1)
    i = np.arange(n, dtype=np.int64)
    cols["ts"] = w.T0 + (i // burst) * gap + (i % burst) * 2
    for s, e in TS_BOUNDS[1:]:
        span = int(cols["ts"][e - 1] - cols["ts"][s])
        assert (1 << 31) < span < (1 << 32)
    return cols


def test_u32_timestamp_offsets(oracle_built):
    check(w.C2_APP, gap_cols(), w.symbols(300), TS_BOUNDS, 101)


# ---- 4. kinds and operators ----------------------------------------------------------------------------------
OPS = {"gt": ">", "ge": ">=", "lt": "<", "le": "<="}
# scan column -> the e1 filter: in the scan's own kind (double, int), on another column (long)
KIND_E1 = {"price": "[price>20]", "id": "[price>20]", "volume": "[volume>100]"}


def kinds_cols():
    n = 10_000
    cols = w.c2_columns(n, keys=37, per_ms=3)
    z = w.splitmix64(99, n)
    price = np.round(cols["price"], 1)  # ties, for >= / <=
    price[np.arange(n) % 53 == 7] = np.nan
    cols["price"] = price
    cols["id"] = (z % np.uint64(1_000_000)).astype(np.int64) - 500_000
    cols["volume"] = ((z >> np.uint64(24)) % np.uint64(300)).astype(np.int32)
    return cols


def kinds_app(col, op, left):
    c1 = "%s %s e1.%s" % (col, OPS[op], col) if left else "e1.%s %s %s" % (col, OPS[op], col)
    return app_of("every e1=StockStream%s -> e2=StockStream[%s] within 1 sec" % (KIND_E1[col], c1))


@pytest.mark.parametrize("left", [True, False], ids=["e2left", "e2right"])
@pytest.mark.parametrize("op", sorted(OPS))
@pytest.mark.parametrize("col", ["price", "id", "volume"])
def test_kinds_and_operators(col, op, left, oracle_built):
    check(kinds_app(col, op, left), kinds_cols(), w.symbols(37), even_bounds(10_000, 3), 101)


EXTRA_APPS = {
    # no e1 filter; a three-column select with an int attribute (the general select loop)
    "nofilter": app_of("every e1=StockStream -> e2=StockStream[price > e1.price] within 200 millisec"),
    "select3": app_of("every e1=StockStream[price>20] -> e2=StockStream[price > e1.price] within 1 sec",
                      " select e1.id as e1id, e2.id as e2id, e2.volume as v"),
}


@pytest.mark.parametrize("case", sorted(EXTRA_APPS))
def test_filter_and_select_shapes(case, oracle_built):
    check(EXTRA_APPS[case], kinds_cols(), w.symbols(37), even_bounds(10_000, 3), 101)


# ---- 5. the other builds of the kernel -----------------------------------------------------------------------
def test_one_key_build(oracle_built):
    cols = w.c1_columns(20_000)
    cols["key"] = np.zeros(len(cols["ts"]), np.int64)
    ref = oracle_c_rows(w.C1_APP, cols)
    assert len(ref) > 100
    assert product_rows(w.C1_APP, cols, ["IBM"], even_bounds(20_000, 3)) == ref


CONST_APP = app_of("every e1=StockStream[price>20] -> e2=StockStream[price > 29.5] within 1 sec")


def other_cols():
    return w.c2_columns(30_000, keys=700, per_ms=3)


def test_constant_scan_build(oracle_built):
    check(CONST_APP, other_cols(), w.symbols(700), even_bounds(30_000, 3), 101)


def test_arrival_order_columns_build(oracle_built, monkeypatch):
    monkeypatch.setenv("SDG_FU_OCOLS", "1")
    check(w.C2_APP, other_cols(), w.symbols(700), even_bounds(30_000, 3), 101)


def _child():
    """(child process of test_run_time_operator_build) the product's rows as JSON on stdout"""
    rows = product_rows(w.C2_APP, other_cols(), w.symbols(700), even_bounds(30_000, 3))
    print("ROWS " + json.dumps([[int(t), [int(x) for x in v]] for t, v in rows]))


def test_run_time_operator_build(oracle_built):
    """SDG_FU_NO_SOP is read once per process, so the product runs in a child process started with it set"""
    ref = oracle_c_rows(w.C2_APP, other_cols(), w.symbols(700))
    assert len(ref) > 100
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, SDG_FU_NO_SOP="1",
               PYTHONPATH=os.pathsep.join([here, os.path.dirname(here), os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-c", "import test_gpu_fused_args as m; m._child()"], env=env, cwd=here,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("ROWS ")][-1]
    got = [(t, tuple(v)) for t, v in json.loads(line[5:])]
    assert got == [(int(t), tuple(int(x) for x in v)) for t, v in ref]
