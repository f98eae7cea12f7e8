"""The launch plan and buffer sizes of the forward / data-gradient implicit GEMM in each of its forms (3x3, sub-pixel forward,
sub-pixel data gradient, K x K): the answers of the workspace, statistics and splits queries and of mnk_last_plan for a sweep of
shapes against tests/golden/fwd_plans.npz (tools/record_fwd_plans.py).  The callers size their workspace and statistics buffers
from these answers and the launch reads the same plan: a rule that changes shows up here, in review, before it shows up as a
buffer of the wrong size."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_fwd_plans as rec  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "fwd_plans.npz")


def _load():
    z = np.load(FIXTURE)
    assert tuple(str(c) for c in z["columns"]) == rec.COLUMNS
    return z["table"]


def _table_keys(header):
    """{(M, Cout, chunks, taps, phases)} of a plan table (csrc/plan_table*.h)"""
    with open(os.path.join(ROOT, "monkey-net_amd", "csrc", header)) as f:
        return set(tuple(int(v) for v in m.groups()) for m in re.finditer(
            r"^\s*\{(\d+), (\d+), (\d+), (\d+), (\d+), \d+, \d+, \d+\},", f.read(), re.M))


def test_fixture_reaches_every_arm():
    """The sweep cannot quietly miss an arm of the planner."""
    t = _load()
    col = {c: t[:, i] for i, c in enumerate(rec.COLUMNS)}
    assert os.path.getsize(FIXTURE) < 1 << 20
    swept = (col["force_bm"] == 0) & (col["force_bn"] == 0) & (col["force_splits"] == 0)
    assert set(int(v) for v in col["form"]) == set(range(len(rec.FORMS)))
    for mode in (0, 1):
        m = swept & (col["gemm_bf16x3"] == mode)
        for bm, bn in rec.TILES:
            assert (m & (col["plan_bm"] == bm) & (col["plan_bn"] == bn)).any(), (mode, bm, bn)
        assert set(int(v) for v in col["plan_phases"][m]) == {1, 4}
        assert (m & (col["plan_splits"] > 1)).sum() > 1000 and (m & (col["plan_splits"] == 1)).sum() > 1000
        # a split plan has a workspace, an un-split one has none; both statistics arms (per M tile / per reduction row block)
        assert (col["ws_floats"][m & (col["plan_splits"] > 1)] > 0).all() and not col["ws_floats"][m & (col["plan_splits"] == 1)].any()
        assert (col["stats_floats"][m & (col["plan_splits"] > 1)] > 0).any() and (col["stats_floats"][m] > 0).all()
    assert ((col["C1"] > 0) & (col["form"] == rec.F_3X3)).any() and ((col["C1"] > 0) & (col["form"] == rec.F_UP)).any()
    has_splits = np.array([f[3] is not None for f in rec.FORMS])[col["form"]]
    assert (col["splits"][has_splits] == col["plan_splits"][has_splits]).all() and (col["splits"][~has_splits] == -1).all()
    # a plan that a plan table supplied (default tuning reads plan_table.h; gemm_bf16x3 its own table, then that one)
    key = list(zip(*(col[c].tolist() for c in ("plan_M", "plan_Cout", "plan_chunks", "plan_taps", "plan_phases"))))
    tables = (_table_keys("plan_table.h"), _table_keys("plan_table_bf16x3.h"))
    assert len(tables[0]) > 10 and len(tables[1]) > 10
    assert any(s and g == 0 and k in tables[0] for s, g, k in zip(swept, col["gemm_bf16x3"], key))
    assert any(s and g == 1 and k in tables[1] for s, g, k in zip(swept, col["gemm_bf16x3"], key))
    # forced tiles: taken, and refused (no kernel is instantiated for the pair, or not for this layer)
    both = (col["force_bm"] > 0) & (col["force_bn"] > 0)
    taken = both & (col["plan_bm"] == col["force_bm"]) & (col["plan_bn"] == col["force_bn"])
    assert taken.sum() > 100 and (both & ~taken).sum() > 100
    ok = set(rec.TILES)
    assert any((int(a), int(b)) in ok for a, b in zip(col["force_bm"][both & ~taken], col["force_bn"][both & ~taken]))
    assert any((int(a), int(b)) not in ok for a, b in zip(col["force_bm"][both], col["force_bn"][both]))
    assert set((int(a), int(b)) for a, b in zip(col["force_bm"][taken], col["force_bn"][taken])) == ok
    forced = col["force_splits"] > 0
    assert (col["plan_splits"][forced] <= col["force_splits"][forced]).all() and (col["plan_splits"][forced] > 1).any()


def test_planner_answers_as_recorded(be):
    t = _load()
    got = rec.answers(be.lib, t[:, :rec.N_IN])
    bad = np.flatnonzero((got != t[:, rec.N_IN:]).any(axis=1))
    assert len(bad) == 0, "%d of %d rows differ; first: %s %s recorded %s now %s" % (
        len(bad), len(t), rec.FORMS[t[bad[0], 0]][0], dict(zip(rec.COLUMNS[1:rec.N_IN], t[bad[0], 1:rec.N_IN].tolist())),
        t[bad[0], rec.N_IN:].tolist(), got[bad[0]].tolist())
