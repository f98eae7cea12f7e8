"""Opt-in evaluation-mode norm fusion at model level (mnk.ops.eval_norm_fusion, Reconstructor / Transfer(fuse_norm=True),
MNK_EVAL_FUSE_NORM): unsplit 3x3 and sub-pixel convolutions apply the frozen norm layer, ReLU and 2x2 average pool behind them
in their own epilogue.  The fused form computes what the default computes -- every comparison here is torch.equal -- so the
tests are about equality, about which conv -> norm pairs ran in which form (ops.EVAL_NORM_COUNT against the library's form
query, the norm-apply launch count of the event recorder), and about everything outside the opt-in staying what it was:
training, gradients, the scope off.

The tiny models' maps are small enough that the default plans split most layers along K (those pairs keep the deferred-split
hand-over); `unsplit` forces one split (force_splits = 1) so that every pair reaches the fused launches."""
import ctypes

import pytest
import torch

from oracle import cases
from test_modules import build, load

RECON = ("video_prediction", "video_deformed", "kp_driving_mean", "kp_source_mean")
NORM_PARAMS = dict(movement_mult=True, move_location=True, adapt_variance=True, clip_mean=True)


def _models(gold, be):
    gen, disc, kpd = build(gold["cfg"])
    gen.load_state_dict(gold["state"]["generator"]), kpd.load_state_dict(gold["state"]["kp_detector"])
    return gen.to(be.device).eval(), kpd.to(be.device).eval()


class _Unsplit:
    """force_splits = 1 (`on`) for the launches inside"""

    def __init__(self, be, on=True):
        self.be, self.on = be, on

    def __enter__(self):
        self.be.lib.call("mnk_set_tuning", b"force_splits", 1 if self.on else 0)

    def __exit__(self, *exc):
        self.be.lib.call("mnk_set_tuning", b"force_splits", 0)


def _flat(out, prefix=""):
    """every tensor of a (nested) result dict by dotted name"""
    flat = {}
    for k, v in out.items():
        if isinstance(v, dict):
            flat.update(_flat(v, prefix + k + "."))
        elif torch.is_tensor(v):
            flat[prefix + k] = v.clone()
    return flat


def _assert_equal(a, b, what):
    a, b = _flat(a), _flat(b)
    assert set(a) == set(b) and a, what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))


def _pairs(be):
    """the library's recorder: {kernel group: launches since the last reset}"""
    lib = be.lib.cdll
    out = {}
    for k in range(lib.mnk_prof_num_kernels()):
        n, ms, work = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double()
        lib.mnk_prof_query(k, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(work))
        name = lib.mnk_prof_kernel_name(k)
        out[name.decode() if isinstance(name, bytes) else name] = n.value
    return out


def _inputs(be, gold, frames=3):
    src, drv = cases.smooth_pair(gold["batch"], gold["size"], gold["size"])
    video = torch.cat([cases.smooth_pair(gold["batch"], gold["size"], gold["size"], seed=20 + i)[1] for i in range(frames)], dim=2)
    return be.t(src), be.t(drv), be.t(video)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "tiny2"])
def test_fused_models_equal_the_default(be, name, precision):
    from mnk import engine, ops
    gold = load(name)
    gen, kpd = _models(gold, be)
    src, drv, video = _inputs(be, gold)
    for unsplit in (True, False):
        with _Unsplit(be, unsplit):
            ops.clear_eval_norm_count()
            want = engine.Reconstructor(kpd, gen, precision=precision)(src, drv)
            assert ops.EVAL_NORM_COUNT[:2] == [0, 0], "the default ran a fused launch"
            got = engine.Reconstructor(kpd, gen, precision=precision, fuse_norm=True)(src, drv)
            be.sync()
            _assert_equal({k: got[k] for k in RECON}, {k: want[k] for k in RECON}, (name, precision, unsplit, "Reconstructor"))
            if unsplit:
                assert ops.EVAL_NORM_COUNT[0] > 0 and ops.EVAL_NORM_COUNT[1] > 0, ("nothing was fused", ops.EVAL_NORM_COUNT)
                for shared in (False, True):
                    want = engine.Transfer(kpd, gen, NORM_PARAMS, shared_source=shared, precision=precision)(src, video)
                    got = engine.Transfer(kpd, gen, NORM_PARAMS, shared_source=shared, precision=precision, fuse_norm=True)(src, video)
                    be.sync()
                    _assert_equal(got, want, (name, precision, "Transfer", shared))
            assert ops.handover_state() == {}, ops.handover_state()
    assert not ops.current_norm_fusion()


def test_counts_of_fused_pairs_and_norm_apply_launches(be, monkeypatch):
    """With one split forced, every DownBlock3D / UpBlock3D / ResBlock3D conv1 -> norm pair of a forward runs fused -- except the
    pooled layers whose form query answers 0, exactly those -- and the norm-apply launches drop by the number of fused pairs.
    With the scope off nothing is fused and every norm layer call is one norm-apply launch, as before."""
    from mnk import engine, ops
    gold = load("tiny2")
    gen, kpd = _models(gold, be)
    src, drv, _ = _inputs(be, gold)
    seen = {"pairs": [], "bn_act": 0}
    conv3x3, bn_act = ops.conv3x3, ops.bn_act

    def spy_conv(x0, c0, weight, *a, **kw):
        follow = kw.get("follow")
        if follow is not None and not torch.is_grad_enabled():
            ups, x1, c1 = kw.get("ups", False), kw.get("x1"), kw.get("c1", 0)
            n, hs, ws = x0.shape[:3]
            up = bool(ups) and bool(ops.subpixel(ups))
            h, w = (hs, ws) if (up or not ups) else (2 * hs, 2 * ws)
            flags = 0 if up else (int(bool(ups)) | 2)
            seen["pairs"].append((be.query("mnk_conv3x3_evalnorm_form", n, h, w, c0, c1, weight.shape[0], flags, int(up), int(follow[2])),
                                  bool(follow[2])))
        return conv3x3(x0, c0, weight, *a, **kw)

    def spy_bn(*a, **kw):
        seen["bn_act"] += 1
        return bn_act(*a, **kw)

    monkeypatch.setattr(ops, "conv3x3", spy_conv)
    monkeypatch.setattr(ops, "bn_act", spy_bn)
    results = {}
    with _Unsplit(be):
        for fuse in (False, True):
            rec = engine.Reconstructor(kpd, gen, fuse_norm=fuse)
            rec(src, drv)                          # (packs and coefficient caches filled: the counted pass launches the forward only)
            be.sync()
            seen["pairs"], seen["bn_act"] = [], 0
            ops.clear_eval_norm_count()
            be.lib.cdll.mnk_prof_reset()
            be.lib.cdll.mnk_prof_enable(1)
            try:
                rec(src, drv)
                be.sync()
            finally:
                be.lib.cdll.mnk_prof_enable(0)
            results[fuse] = (list(ops.EVAL_NORM_COUNT), _pairs(be)["bn_act_apply"], list(seen["pairs"]), seen["bn_act"])
            be.lib.cdll.mnk_prof_reset()
    (count0, apply0, pairs0, calls0), (count1, apply1, pairs1, calls1) = results[False], results[True]
    print("pairs", len(pairs1), "forms", [sum(1 for f, _ in pairs1 if f == k) for k in (0, 1, 2)], "counts off / on", count0, count1,
          "norm-apply launches off / on", apply0, apply1, "bn_act calls", calls0)
    assert pairs0 == pairs1 and calls0 == calls1 and len(pairs1) >= 10
    n = [sum(1 for f, _ in pairs1 if f == k) for k in (0, 1, 2)]
    assert n[1] > 0 and n[2] > 0
    assert all(pool for f, pool in pairs1 if f == 0), "only pooled layers may lack a fused form when nothing splits"
    # scope on: every pair fused in the form the query names, none deferred, the rest (form 0) separate
    assert count1 == [n[1], n[2], 0, n[0]], (count1, n)
    assert apply0 - apply1 == n[1] + n[2], (apply0, apply1, n)
    # scope off: nothing fused, and one norm-apply launch per norm layer call
    assert count0 == [0, 0, 0, len(pairs0)], count0
    assert apply0 == calls0, (apply0, calls0)


def test_default_plans_defer_split_pairs_as_before(be):
    """with nothing forced the tiny maps split along K: those pairs keep the deferred-split launch inside the scope too"""
    from mnk import engine, ops
    gold = load("tiny")
    gen, kpd = _models(gold, be)
    src, drv, _ = _inputs(be, gold)
    counts = {}
    for fuse in (False, True):
        rec = engine.Reconstructor(kpd, gen, fuse_norm=fuse)
        ops.clear_eval_norm_count()
        rec(src, drv)
        be.sync()
        counts[fuse] = list(ops.EVAL_NORM_COUNT)
    assert counts[False][:2] == [0, 0] and counts[False][2] > 0
    assert counts[True][2] == counts[False][2], counts
    assert sum(counts[True]) == sum(counts[False]), counts


def test_scope_semantics_and_gradients_take_the_unfused_path(be):
    from mnk import ops
    gold = load("tiny")
    gen, kpd = _models(gold, be)
    src, drv, _ = _inputs(be, gold)
    assert not ops.current_norm_fusion()
    with ops.eval_norm_fusion(True):
        assert ops.current_norm_fusion()
        with ops.eval_norm_fusion(False):
            assert not ops.current_norm_fusion()
        assert ops.current_norm_fusion()
    with pytest.raises(ZeroDivisionError):
        with ops.eval_norm_fusion(True):
            1 / 0
    assert not ops.current_norm_fusion()

    def grads(fuse):
        kpd.zero_grad()
        with _Unsplit(be), ops.eval_norm_fusion(fuse):
            ops.clear_eval_norm_count()
            out = kpd(drv)["mean"]                      # evaluation-mode norm layers, gradients enabled
            assert ops.EVAL_NORM_COUNT == [0, 0, 0, 0], "a pair was counted (or fused) with gradients enabled"
            out.square().sum().backward()
        be.sync()
        return out.detach().clone(), [p.grad.clone() for p in kpd.parameters() if p.grad is not None]

    out0, g0 = grads(False)
    out1, g1 = grads(True)
    assert torch.equal(out0, out1) and len(g0) == len(g1) > 0
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    # a training-mode norm layer inside the scope, under no_grad: batch statistics, nothing fused
    kpd.train()
    try:
        with torch.no_grad(), _Unsplit(be):
            ops.clear_eval_norm_count()
            a = kpd(drv)["mean"].clone()
            with ops.eval_norm_fusion(True):
                b = kpd(drv)["mean"].clone()
            assert ops.EVAL_NORM_COUNT == [0, 0, 0, 0]
    finally:
        kpd.eval()
    be.sync()
    assert ops.handover_state() == {}


def test_one_training_step_inside_the_scope_equals_the_step_outside(be):
    from mnk import engine, ops
    cfg = cases.TINY
    src, drv = cases.smooth_pair(4, 32, 32)
    results = []
    for fuse in (False, True):
        gen, disc, kpd = build(cfg)
        for i, m in enumerate((gen, disc, kpd)):
            sd = m.state_dict()
            cases.perturb_state_dict(sd, 7 + i)
            m.load_state_dict(sd)
        gen.to(be.device), disc.to(be.device), kpd.to(be.device)
        step = engine.TrainStep(gen, disc, kpd, cfg["train_params"])
        with ops.eval_norm_fusion(fuse):
            ops.clear_eval_norm_count()
            g_losses, d_losses, generated = step.step({"source": be.t(src), "video": be.t(drv)})
            be.sync()
            assert ops.EVAL_NORM_COUNT[:2] == [0, 0]
        results.append(([float(v) for v in g_losses], [float(v) for v in d_losses], generated["video_prediction"].detach().clone(),
                        [p.detach().clone() for m in (gen, disc, kpd) for p in m.parameters()]))
    a, b = results
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2])
    for p, q in zip(a[3], b[3]):
        assert torch.equal(p, q)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_captured_graph_keeps_the_form_it_was_built_with(precision):
    from conftest import Backend
    from mnk import engine, ops
    be = Backend("hip")
    gold = load("tiny2")
    gen, kpd = _models(gold, be)
    src, drv, _ = _inputs(be, gold)
    with _Unsplit(be):
        eager = engine.Reconstructor(kpd, gen, precision=precision)
        fused = engine.Reconstructor(kpd, gen, precision=precision, fuse_norm=True, use_graph=True)
        plain = engine.Reconstructor(kpd, gen, precision=precision, use_graph=True)
        for it in range(2):
            s, d = (src, drv) if it == 0 else (drv, src)
            want = {k: v.clone() for k, v in eager(s, d).items()}
            ops.clear_eval_norm_count()
            got = fused(s, d)                      # replays launch nothing from Python: the counter stays at zero after the capture
            torch.cuda.synchronize()
            _assert_equal({k: got[k] for k in RECON}, want, ("graph, fused", it))
            if it:
                assert ops.EVAL_NORM_COUNT == [0, 0, 0, 0]
            got = plain(s, d)
            torch.cuda.synchronize()
            _assert_equal({k: got[k] for k in RECON}, want, ("graph, default", it))
    assert ops.handover_state() == {}


@pytest.mark.gpu
def test_eval_runner_captures_one_program_per_form(monkeypatch):
    """the reference's per-frame loop behind DataParallelWithCallback: MNK_EVAL_FUSE_NORM=1 gives the frames of =0, and changing
    the variable captures a program of its own instead of replaying the other form"""
    from conftest import Backend
    from sync_batchnorm import DataParallelWithCallback
    from mnk import dropin, ops
    be = Backend("hip")
    gold = load("tiny2")
    gen, kpd = _models(gold, be)
    generator, kp_detector = DataParallelWithCallback(gen), DataParallelWithCallback(kpd)
    generator.eval(), kp_detector.eval()
    src, drv, _ = _inputs(be, gold)
    src, drv = src[:1], drv[:1]
    monkeypatch.delenv("MNK_EVAL_PRECISION", raising=False)
    frames = {}
    with torch.no_grad(), _Unsplit(be):
        for value, captures in (("0", 1), ("1", 2), ("0", 2), ("1", 2)):
            monkeypatch.setenv("MNK_EVAL_FUSE_NORM", value)
            for _ in range(2):
                kp_source, kp_driving = kp_detector(src), kp_detector(drv)
                out = generator(source_image=src, kp_driving=kp_driving, kp_source=kp_source)["video_prediction"]
                torch.cuda.synchronize()
                frames.setdefault(value, out.clone())
                assert torch.equal(out, frames["0"]), value
                runner = dropin.eval_runner_for_wrapper(generator)
                assert runner is not None and runner.stats["captures"] == captures, (value, runner.stats)
        # the eager fall-back follows the variable too, and an enclosing scope has precedence over it
        monkeypatch.setenv("MNK_EVAL_GRAPH", "0")
        for value, scope, fused in (("0", False, False), ("1", False, True), ("0", True, True)):
            monkeypatch.setenv("MNK_EVAL_FUSE_NORM", value)
            ops.clear_eval_norm_count()
            with ops.eval_norm_fusion(scope):
                out = kp_detector(drv)["mean"]
            torch.cuda.synchronize()
            assert (ops.EVAL_NORM_COUNT[0] + ops.EVAL_NORM_COUNT[1] > 0) == fused, (value, scope, ops.EVAL_NORM_COUNT)
    assert not ops.current_norm_fusion()
