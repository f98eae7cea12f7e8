#!/usr/bin/env python
"""Record what the forward / data-gradient launch planner decides for a sweep of shapes: tests/golden/fwd_plans.npz, the
fixture of tests/test_fwd_plans.py.  The planner is host code, so the CPU emulator build of the library answers (no GPU needed).

A row is a form (FORMS), the arguments of its size queries (N, H, W, C0, C1, Cout), the tuning values it was asked under
(gemm_bf16x3, force_bm, force_bn, force_splits; everything else at its default) and the answers: the workspace floats, the
statistics floats, the splits (-1: the form has no such query) and the eight values of mnk_last_plan after the workspace query.
Re-record ONLY when a plan rule, a plan table or a tuning default is changed on purpose; the diff of the fixture's summary
(printed here) is then what a reviewer looks at.

Usage: tools/record_fwd_plans.py [--library libmnk_emu.so] [--out tests/golden/fwd_plans.npz]"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "monkey-net_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

COLUMNS = ("form", "N", "H", "W", "C0", "C1", "Cout", "gemm_bf16x3", "force_bm", "force_bn", "force_splits",
           "ws_floats", "stats_floats", "splits",
           "plan_M", "plan_Cout", "plan_chunks", "plan_taps", "plan_phases", "plan_bm", "plan_bn", "plan_splits")
N_IN = 11
TUNING = ("gemm_bf16x3", "force_bm", "force_bn", "force_splits")      # columns 7 .. 10
# form -> (workspace query, statistics query, splits query or None, arguments of the three from a row's N, H, W, C0, C1, Cout)
FORMS = (
    ("3x3", "mnk_conv3x3_workspace_floats", "mnk_conv3x3_stats_floats", "mnk_conv3x3_splits",
     lambda n, h, w, c0, c1, cout: (n, h, w, c0, c1, cout)),
    # (H, W) = the LOW resolution
    ("sub-pixel forward", "mnk_conv3x3_up_workspace_floats", "mnk_conv3x3_up_stats_floats", "mnk_conv3x3_up_splits",
     lambda n, h, w, c0, c1, cout: (n, h, w, c0, c1, cout)),
    # dy has C0 channels, dx (N, H, W) has Cout: the GEMM's own reading of the two counts
    ("sub-pixel data gradient", "mnk_conv3x3_up_dgrad_workspace_floats", "mnk_conv3x3_up_dgrad_stats_floats", None,
     lambda n, h, w, c0, c1, cout: (n, h, w, c0, cout)),
    ("4x4", "mnk_conv2d_workspace_floats", "mnk_conv2d_stats_floats", None,
     lambda n, h, w, c0, c1, cout: (n, h, w, c0, c1, cout, 16)),
)
F_3X3, F_UP, F_UP_DGRAD, F_4X4 = range(4)
TILES = ((128, 16), (128, 32), (128, 48), (64, 64), (128, 64), (64, 128), (128, 128))       # (bm, bn)


def shapes():
    """record_wgrad_plans.sweep()'s jobs as distinct (N, H, W, C, Cout, taps, up-sampled); (H, W) = the output map"""
    import record_wgrad_plans as wg
    j = wg.sweep()
    return sorted(set((int(r[0]), int(r[1]), int(r[2]), int(r[5]), int(r[6]), int(r[7] * r[8]), int(r[12]) & 1) for r in j))


def forms_of(n, h, w, c, cout, taps, ups):
    """every form the shape can take: (form, N, H, W, C0, C1, Cout)"""
    if taps == 16:                       # 4x4 / pad 0 forward, and its data gradient (4x4 / pad 3) at the input size
        return [(F_4X4, n, h, w, c, 0, cout), (F_4X4, n, h + 3, w + 3, cout, 0, c)]
    out = [(F_3X3, n, h, w, c, 0, cout), (F_3X3, n, h, w, cout, 0, c)]          # forward; data gradient: channels swapped
    if ups and h % 2 == 0 and w % 2 == 0:
        out += [(F_UP, n, h // 2, w // 2, c, 0, cout), (F_UP_DGRAD, n, h // 2, w // 2, cout, 0, c)]
    return out


def sweep():
    import test_kernels_conv as kc
    base = [f for s in shapes() for f in forms_of(*s)]
    rows = [f + (mode, 0, 0, 0) for mode in (0, 1) for f in base]
    # two sources (the decoder's skip connections): the kernel tests' cases
    for n, h, w, c0, c1, cout, ups, _, _ in kc.CASES + kc.HALO_CASES + kc.COMPACT_CASES:
        if c1:
            for mode in (0, 1):
                rows.append((F_3X3, n, h, w, c0, c1, cout, mode, 0, 0, 0))
                if ups:
                    rows.append((F_UP, n, h, w, c0, c1, cout, mode, 0, 0, 0))
    # forced plans: every tile (and pairs no kernel is instantiated for, which the planner refuses) and split counts on a few
    # shapes of every form
    forced = [(F_3X3, 2, 16, 16, 40, 0, 10), (F_3X3, 4, 32, 32, 64, 0, 45), (F_3X3, 1, 8, 8, 136, 0, 128),
              (F_3X3, 8, 64, 64, 35, 0, 256), (F_UP, 2, 8, 8, 72, 0, 40), (F_UP, 4, 16, 16, 64, 64, 130),
              (F_UP_DGRAD, 2, 16, 16, 45, 0, 70), (F_4X4, 2, 13, 13, 13, 0, 64), (F_4X4, 8, 29, 29, 128, 0, 16)]
    for f in forced:
        for mode in (0, 1):
            for bm, bn in TILES + ((64, 32), (64, 16), (32, 64), (128, 96), (0, 64), (64, 0), (128, 0), (0, 16)):
                for splits in (0, 3):
                    rows.append(f + (mode, bm, bn, splits))
            for splits in (1, 2, 7, 1000):
                rows.append(f + (mode, 0, 0, splits))
    # (no duplicates removed: a layer's data gradient may be another layer's forward; the row count is forms x shapes)
    return np.array(rows, dtype=np.int64)


def answers(lib, rows):
    """The planner's answers for `rows` (the first N_IN columns): an int64 array of 11 columns per row.
    lib: a mnk._lib.Library."""
    out = np.zeros((len(rows), len(COLUMNS) - N_IN), dtype=np.int64)
    before = []
    for name in TUNING:
        v = ctypes.c_int(0)
        lib.call("mnk_get_tuning", name.encode(), ctypes.byref(v))
        before.append(v.value)
    plan = (ctypes.c_long * 8)()
    try:
        for tuning in sorted(set(tuple(int(v) for v in r) for r in rows[:, 7:N_IN])):
            for name, v in zip(TUNING, tuning):
                lib.call("mnk_set_tuning", name.encode(), v)
            for i in np.flatnonzero((rows[:, 7:N_IN] == np.array(tuning)).all(axis=1)):
                form, n, h, w, c0, c1, cout = (int(v) for v in rows[i, :7])
                _, q_ws, q_stats, q_splits, argsof = FORMS[form]
                args = argsof(n, h, w, c0, c1, cout)
                out[i, 1] = lib.query(q_stats, *args)
                out[i, 2] = lib.query(q_splits, *args) if q_splits else -1
                out[i, 0] = lib.query(q_ws, *args)
                if lib.query("mnk_last_plan", plan) != 0:
                    raise RuntimeError("mnk_last_plan failed")
                out[i, 3:] = list(plan)
    finally:
        for name, v in zip(TUNING, before):
            lib.call("mnk_set_tuning", name.encode(), v)
    return out


def summary(table):
    col = {c: table[:, i] for i, c in enumerate(COLUMNS)}
    swept = (col["force_bm"] == 0) & (col["force_bn"] == 0) & (col["force_splits"] == 0)
    parts = ["%d rows, %d of them with a forced plan" % (len(table), int((~swept).sum()))]
    for mode in (0, 1):
        m = swept & (col["gemm_bf16x3"] == mode)
        tiles = {"%dx%d" % t: int((m & (col["plan_bm"] == t[0]) & (col["plan_bn"] == t[1])).sum()) for t in TILES}
        parts.append("gemm_bf16x3=%d: %d rows, split %d, un-split %d, tiles %s" % (
            mode, int(m.sum()), int((m & (col["plan_splits"] > 1)).sum()), int((m & (col["plan_splits"] == 1)).sum()), tiles))
    return "; ".join(parts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--library", default=os.path.join(ROOT, "tests", "hipemu", "build", "libmnk_emu.so"),
                    help="the build that answers (default: this tree's CPU emulator build, tests/hipemu/build.sh)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "fwd_plans.npz"))
    args = ap.parse_args()
    from mnk import _lib
    lib = _lib.Library(args.library, strict=False)
    rows = sweep()
    table = np.concatenate([rows, answers(lib, rows)], axis=1)
    np.savez_compressed(args.out, columns=np.array(COLUMNS), table=table)
    print("%d shapes; %s" % (len(shapes()), summary(table)))
    print(args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
