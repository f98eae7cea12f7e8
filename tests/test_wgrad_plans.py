"""Which weight-gradient form a layer runs, with how many splits and how many floats of partials: the answers of
mnk_conv2d_wgrad_plan2 and mnk_wgrad_grouped_plan for a sweep of jobs against tests/golden/wgrad_plans.npz
(tools/record_wgrad_plans.py).  The callers size their partial buffers from these answers, and the launches write what the
same selection computes: a split rule that changes shows up here, in review, before it shows up as a wrong buffer size."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_wgrad_plans as rec  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "wgrad_plans.npz")


def _load():
    z = np.load(FIXTURE)
    assert tuple(str(c) for c in z["columns"]) == rec.COLUMNS
    return z["table"]


def test_fixture_reaches_every_form():
    """The sweep cannot quietly miss an arm of the selection."""
    t = _load()
    col = {c: t[:, i] for i, c in enumerate(rec.COLUMNS)}
    assert len(t) >= 5000 and os.path.getsize(FIXTURE) < 1 << 20
    assert set(int(v) for v in col["plan_layout"]) == {0, 1, 2}
    assert (col["plan_splits"] == 0).sum() > 100 and (col["plan_splits"] > 0).sum() > 100
    v = col["grouped_variant"]
    tap = v[(v >= 0) & (v < 16)]
    for tile in range(4):           # 128x128, 128x64, 64x128, 32x128; loaders: generic, 3x3 buffer loads, sub-pixel
        assert {0, 1, 3} <= set(int(x) % 4 for x in tap if int(x) // 4 == tile), tile
    assert 2 in set(int(x) % 4 for x in tap)            # the up-sampled view's loader: only with up_subpixel = 0
    assert set(int(x) for x in col["up_subpixel"][(v >= 0) & (v < 16) & (v % 4 == 2)]) == {0}
    assert len(set(int(x) for x in v[v >= 16])) >= 2 and int(v.max()) < 25
    assert ((v == -1) & (col["plan_layout"] == 1)).any() and ((v == -1) & (col["plan_splits"] == 0)).any()
    # a job the grouped launch does not take plans nothing there; one it takes leaves tap-major partials
    assert not col["grouped_splits"][v < 0].any() and not col["grouped_part_floats"][v < 0].any()
    assert (col["grouped_splits"][v >= 0] > 0).all()
    # ld_x: round_up(C, 4), round_up(C, 16) and strides that are no multiple of 4
    assert (col["ld_x"] % 4 != 0).any() and (col["ld_x"] == (col["C"] + 15) // 16 * 16).any()
    assert ((col["kh"] == 4) & (col["pad"] == 0)).any()
    # one known shape each of the forms the answers cannot tell apart
    for form, (n, h, w, c, cout) in rec.KNOWN_FORMS.items():
        hit = (col["N"] == n) & (col["Ho"] == h) & (col["Wo"] == w) & (col["C"] == c) & (col["Cout"] == cout) & \
            (col["ld_x"] == (c + 3) // 4 * 4) & (col["flags"] == 0)
        assert hit.sum() == 1, form
        layout, splits, variant = (int(col[k][hit][0]) for k in ("plan_layout", "plan_splits", "grouped_variant"))
        assert splits > 1 and (layout, variant >= 16) == ((0, True) if form == "nine-tap" else (1, False)), form


def test_planners_answer_as_recorded(be):
    t = _load()
    got = rec.answers(be.lib, t[:, :rec.N_IN])
    bad = np.flatnonzero((got != t[:, rec.N_IN:]).any(axis=1))
    assert len(bad) == 0, "%d of %d rows differ; first: job %s recorded %s now %s" % (
        len(bad), len(t), dict(zip(rec.COLUMNS[:rec.N_IN], t[bad[0], :rec.N_IN].tolist())),
        t[bad[0], rec.N_IN:].tolist(), got[bad[0]].tolist())


def test_grouped_plan_reports_the_layout(be):
    """MnkWgradJob::layout: 2 for the sub-pixel form's 16 pseudo taps, else 0 -- what mnk_wgrad_reduce_multi is told."""
    from mnk.optim import JOB
    t = _load()
    t = t[t[:, 13] == 1]
    jobs = np.zeros(len(t), dtype=JOB)
    for f, c in (("N", 0), ("Ho", 1), ("Wo", 2), ("Hi", 3), ("Wi", 4), ("C", 5), ("Cout", 6), ("kh", 7), ("kw", 8), ("pad", 9),
                 ("ld_x", 10), ("ld_dy", 11), ("flags", 12)):
        jobs[f] = t[:, c]
    jobs["layout"] = -7
    assert be.query("mnk_wgrad_grouped_plan", jobs.ctypes.data, len(jobs)) == 0
    v = jobs["variant"]
    assert (jobs["layout"] == np.where((v >= 0) & (v < 16) & (v % 4 == 3), 2, 0)).all()
