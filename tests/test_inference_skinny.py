"""Opt-in weight-streaming convolutions at model level (mnk.ops.eval_skinny_conv, Reconstructor / Transfer(skinny=True),
MNK_EVAL_SKINNY): under no_grad, conv -> evaluation-mode norm pairs whose output has at most `skinny_rows` rows -- the deep
hourglass levels of a batch-1 frame -- run as mnk_conv3x3_skinny_fwd + mnk_bn_eval_split_fwd.

* batch-1 outputs of Reconstructor(skinny=True) against the references the default path is held to: fp32 against the golden's
  eval64 with the tolerances of tests/test_inference.py; bf16 against eval64 with the criterion of tests/test_inference_bf16.py
  (at most twice the error of the fp64 restatement with bf16-rounded 3x3 operands) -- the skinny form rounds the same operands;
* ops.EVAL_SKINNY_COUNT equals the number of pairs with at most skinny_rows output rows, counted from the shapes the model's
  own conv3x3 calls carry;
* the default (no argument, skinny=False) takes no such launch and is bit-equal to a call made before the scope was ever on;
  a batched call has no layer under the threshold; with gradients enabled the scope does nothing;
* (MI355X) EvalRunner: MNK_EVAL_SKINNY is part of the program key, a replay equals the eager skinny forward bit for bit, and a
  load_state_dict is followed (the packs are re-made)."""
import ctypes

import pytest
import torch

from oracle import cases, restate
from test_modules import build, load
import test_inference_bf16 as tb

ROWS = 16                                 # skinny_rows of these tests, whatever the library's default
RECON = ("video_prediction", "video_deformed", "kp_driving_mean", "kp_source_mean")
NORM_PARAMS = dict(movement_mult=True, move_location=True, adapt_variance=True, clip_mean=True)


def _models(gold, be):
    gen, disc, kpd = build(gold["cfg"])
    gen.load_state_dict(gold["state"]["generator"]), kpd.load_state_dict(gold["state"]["kp_detector"])
    return gen.to(be.device).eval(), kpd.to(be.device).eval()


class _Tuned:
    """skinny_rows = ROWS and no class of up-sampled layers excluded (skinny_up_min_weights = 0: the tiny models' weight streams
    are all short), so that every pair at or under ROWS rows takes the form; the library's values are put back"""
    KNOBS = ((b"skinny_rows", ROWS), (b"skinny_up_min_weights", 0))

    def __init__(self, be):
        self.be, self.saved = be, []

    def __enter__(self):
        for k, v in self.KNOBS:
            old = ctypes.c_int(0)
            self.be.lib.cdll.mnk_get_tuning(k, ctypes.byref(old))
            self.saved.append((k, old.value))
            self.be.lib.call("mnk_set_tuning", k, v)
        return self.be

    def __exit__(self, *exc):
        for k, v in self.saved:
            self.be.lib.call("mnk_set_tuning", k, v)


@pytest.fixture
def rows16(be):
    with _Tuned(be):
        yield be


class _PairSpy:
    """the output rows of every conv -> norm pair a forward announces under no_grad (conv3x3(follow=...))"""

    def __init__(self, monkeypatch):
        from mnk import ops
        self.rows = []
        real = ops.conv3x3

        def spy(x0, c0, weight, *a, **kw):
            follow = kw.get("follow")
            if follow is not None and not follow[0].training and not torch.is_grad_enabled() and kw.get("residual") is None:
                n, hs, ws = x0.shape[:3]
                h, w = (2 * hs, 2 * ws) if kw.get("ups", False) else (hs, ws)
                self.rows.append((n * h * w, h % 2 == 0 and w % 2 == 0))
            return real(x0, c0, weight, *a, **kw)

        monkeypatch.setattr(ops, "conv3x3", spy)

    def under(self, limit):
        return sum(1 for r, even in self.rows if r <= limit and even)


def _clone(out, keys=RECON):
    return {k: out[k].clone() for k in keys}


def _assert_equal(a, b, what):
    assert set(a) == set(b) and a, what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k] - b[k]).abs().max()))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_reconstructor_batch1_skinny_outputs_and_count(rows16, monkeypatch, precision):
    from mnk import engine, ops
    be = rows16
    gold = load("tiny")
    gen, kpd = _models(gold, be)
    src, drv = cases.smooth_pair(gold["batch"], gold["size"], gold["size"])
    want = tb._gold_outputs(gold)
    if precision == "bf16":
        monkeypatch.setattr(restate, "conv", tb._rounded_conv)
        rounded = tb._restated(gold["state"], gold["cfg"], src, drv)
        monkeypatch.undo()
        e_ref = {k: tb._err(rounded[k], want[k]) for k in tb.OUTPUTS}
    assert not ops.current_skinny_conv()
    default = engine.Reconstructor(kpd, gen, precision=precision)
    skinny = engine.Reconstructor(kpd, gen, precision=precision, skinny=True)
    spy = _PairSpy(monkeypatch)
    outs = []
    for b in range(gold["batch"]):                       # the frames of the golden batch, one at a time
        s, d = be.t(src[b:b + 1]), be.t(drv[b:b + 1])
        ops.clear_eval_skinny_count()
        before = _clone(default(s, d))
        assert ops.EVAL_SKINNY_COUNT[0] == 0, "the default took a skinny launch"
        spy.rows = []
        ops.clear_eval_norm_count()
        got = _clone(skinny(s, d))
        be.sync()
        expect = spy.under(ROWS)
        print("skinny %s %s frame %d: %d of %d conv -> norm pairs at or under %d rows" % (be.kind, precision, b, expect, len(spy.rows), ROWS))
        assert ops.EVAL_SKINNY_COUNT[0] == expect > 0, (ops.EVAL_SKINNY_COUNT, expect)
        assert sum(ops.EVAL_NORM_COUNT) == len(spy.rows), "every pair is still counted once"
        assert not ops.current_skinny_conv() and ops.handover_state() == {}
        # skinny=False and no argument: no such launch, and the bits of the call made before the scope was ever entered
        ops.clear_eval_skinny_count()
        for rec in (default, engine.Reconstructor(kpd, gen, precision=precision, skinny=False)):
            _assert_equal(_clone(rec(s, d)), before, ("default after the scope", precision, b))
        assert ops.EVAL_SKINNY_COUNT[0] == 0
        outs.append(got)
    out = {k: torch.cat([o[k] for o in outs]).cpu() for k in RECON}
    if precision == "fp32":                              # tests/test_inference.py's tolerances against the golden
        ref = gold["eval64"]
        assert float((out["video_prediction"].double() - ref["video_prediction"].double()).abs().max()) < 2e-5
        assert float((out["video_deformed"].double() - ref["video_deformed"].double()).abs().max()) < 1e-4
        assert float((out["kp_driving_mean"].double() - ref["kp_mean"][:, 1:].double()).abs().max()) < 2e-6
        assert float((out["kp_source_mean"].double() - ref["kp_mean"][:, :1].double()).abs().max()) < 2e-6
        l1 = float((out["video_prediction"].double() - drv.double()).abs().mean())
        l1_ref = float((ref["video_prediction"].double() - drv.double()).abs().mean())
        assert abs(l1 - l1_ref) < 1e-4
    else:                                                # tests/test_inference_bf16.py's criterion
        ratios = {k: tb._err(out[k], want[k]) / e_ref[k] for k in tb.OUTPUTS}
        print("skinny bf16 %s: max |out - eval64| / e_ref %s" % (be.kind, {k: "%.3f" % v for k, v in ratios.items()}))
        for k in tb.OUTPUTS:
            assert e_ref[k] > 1e-6 and ratios[k] <= 2.0, (k, ratios[k], e_ref[k])


def test_batched_transfer_has_no_layer_under_the_threshold(rows16, monkeypatch):
    from mnk import engine, ops
    be = rows16
    gold = load("tiny")
    gen, kpd = _models(gold, be)
    src, _ = cases.smooth_pair(gold["batch"], gold["size"], gold["size"])
    video = torch.cat([cases.smooth_pair(gold["batch"], gold["size"], gold["size"], seed=20 + i)[1] for i in range(3)], dim=2)
    src, video = be.t(src), be.t(video)
    want = engine.Transfer(kpd, gen, NORM_PARAMS)(src, video)
    spy = _PairSpy(monkeypatch)
    ops.clear_eval_skinny_count()
    got = engine.Transfer(kpd, gen, NORM_PARAMS, skinny=True)(src, video)
    be.sync()
    assert spy.rows and spy.under(ROWS) == 0, "this call was meant to have every layer above the threshold"
    assert ops.EVAL_SKINNY_COUNT[0] == 0
    for k in ("video_prediction", "video_deformed"):
        assert torch.equal(got[k], want[k]), k
    for k in ("kp_driving", "kp_source", "kp_norm"):
        _assert_equal(dict(got[k]), dict(want[k]), k)


def test_gradients_enabled_the_scope_does_nothing(rows16):
    from mnk import ops
    be = rows16
    gold = load("tiny")
    gen, kpd = _models(gold, be)
    _, drv = cases.smooth_pair(1, gold["size"], gold["size"])
    drv = be.t(drv)

    def grads(on):
        kpd.zero_grad()
        with ops.eval_skinny_conv(on):
            assert ops.current_skinny_conv() == on
            ops.clear_eval_skinny_count()
            out = kpd(drv)["mean"]                      # evaluation-mode norm layers, batch 1, gradients enabled
            assert ops.EVAL_SKINNY_COUNT[0] == 0, "a skinny launch with gradients enabled"
            out.square().sum().backward()
        be.sync()
        return out.detach().clone(), [p.grad.clone() for p in kpd.parameters() if p.grad is not None]

    out0, g0 = grads(False)
    out1, g1 = grads(True)
    assert torch.equal(out0, out1) and len(g0) == len(g1) > 0
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    with pytest.raises(ZeroDivisionError):
        with ops.eval_skinny_conv(True):
            1 / 0
    assert not ops.current_skinny_conv() and ops.handover_state() == {}


@pytest.mark.gpu
def test_eval_runner_captures_a_program_of_its_own_replays_it_and_follows_a_checkpoint(monkeypatch):
    from conftest import Backend
    from sync_batchnorm import DataParallelWithCallback
    from mnk import dropin, ops
    be = Backend("hip")
    with _Tuned(be):
        gold = load("tiny")
        gen, kpd = _models(gold, be)
        kp_detector = DataParallelWithCallback(kpd)
        kp_detector.eval()
        _, drv = cases.smooth_pair(1, gold["size"], gold["size"])
        drv = be.t(drv)
        monkeypatch.delenv("MNK_EVAL_PRECISION", raising=False)
        monkeypatch.delenv("MNK_EVAL_FUSE_NORM", raising=False)

        def eager(on):
            ops.clear_eval_skinny_count()
            with torch.no_grad(), ops.eval_skinny_conv(on):
                out = {k: t.clone() for k, t in kpd(drv).items()}
            torch.cuda.synchronize()
            assert (ops.EVAL_SKINNY_COUNT[0] > 0) == on
            return out

        frames = {}
        with torch.no_grad():
            for value, captures in (("0", 1), ("1", 2), ("0", 2), ("1", 2)):
                monkeypatch.setenv("MNK_EVAL_SKINNY", value)
                for _ in range(2):
                    out = {k: t.clone() for k, t in kp_detector(drv).items()}
                    torch.cuda.synchronize()
                    runner = dropin.eval_runner_for_wrapper(kp_detector)
                    assert runner is not None and runner.stats["captures"] == captures, (value, runner.stats)
                    _assert_equal(out, eager(value == "1"), ("replay against the eager forward", value))
                    frames.setdefault(value, out)
            # another checkpoint: the next call re-captures, on packs made from the new weights
            sd = {k: t.detach().cpu().clone() for k, t in kpd.state_dict().items()}
            cases.perturb_state_dict(sd, 99, scale=0.05)
            kpd.load_state_dict(sd)
            out = {k: t.clone() for k, t in kp_detector(drv).items()}
            torch.cuda.synchronize()
            assert runner.stats["captures"] == 3
            _assert_equal(out, eager(True), "after load_state_dict")
            assert not torch.equal(out["mean"], frames["1"]["mean"])
        assert not ops.current_skinny_conv()
