"""mnk.engine.AnimationSession: one source, a driving video pushed in chunks (demo.py:60-71, transfer.py:65-79).

The `tiny` golden's models and the inputs of test_batched_transfer_equals_the_frame_loop_and_normalize_kp_its_formulas, with five
driving frames, B = 2, all four normalisation options.  The comparison paths are pinned to the reference elsewhere:
mnk.engine.Transfer by test_inference.py / test_dropin_reference.py, the multi-frame generator by test_multiframe_generator.py.

Bounds: frames 2e-6 -- the project's bound for the same frames through different batchings (test_multiframe_generator.py,
test_inference.py); kp_norm 4e-6 -- both paths are within 2e-6 of the fp64 restatement (test_inference.py)."""
import pytest
import torch

from oracle import cases
from test_modules import load, build

OUTPUTS = ("video_prediction", "video_deformed")
PARAMS = dict(movement_mult=True, move_location=True, adapt_variance=True, clip_mean=True)
FRAMES, KP = 2e-6, 4e-6
D = 5


def bits(t):
    return t.contiguous().cpu().view(torch.int32)


_SHARED = {}


def _setup(be):
    """models, inputs and the whole-video Transfer(shared_source=True) result: made once per backend, never written to"""
    if be.kind not in _SHARED:
        from mnk import engine
        gold = load("tiny")
        gen, _, kpd = build(gold["cfg"])
        gen.load_state_dict(gold["state"]["generator"]), kpd.load_state_dict(gold["state"]["kp_detector"])
        gen.to(be.device).eval(), kpd.to(be.device).eval()
        size = gold["size"]
        src = be.t(cases.smooth_pair(2, size, size, seed=11)[0])
        driving = be.t(torch.cat([cases.smooth_pair(2, size, size, seed=20 + i)[1] for i in range(D)], dim=2))
        whole = engine.Transfer(kpd, gen, PARAMS, shared_source=True)(src, driving)
        be.sync()
        _SHARED[be.kind] = (gen, kpd, src, driving, whole, size)
    return _SHARED[be.kind]


def _keep(out):
    """a captured push (the default on a device build) returns static buffers that the next push of that shape overwrites"""
    return {k: (v.clone() if torch.is_tensor(v) else {kk: t.clone() for kk, t in v.items()}) for k, v in out.items()}


def _pushes(session, driving, splits):
    parts, at = [], 0
    for n in splits:
        parts.append(_keep(session.push(driving[:, :, at:at + n])))
        at += n
    assert at == driving.shape[2]
    return {"video_prediction": torch.cat([p["video_prediction"] for p in parts], dim=2),
            "video_deformed": torch.cat([p["video_deformed"] for p in parts], dim=2),
            "kp_driving": {k: torch.cat([p["kp_driving"][k] for p in parts], dim=1) for k in parts[0]["kp_driving"]},
            "kp_norm": {k: torch.cat([p["kp_norm"][k] for p in parts], dim=1) for k in parts[0]["kp_norm"]},
            "kp_source": parts[0]["kp_source"]}


def _gap(a, b):
    return float((a - b).abs().max())


def _check(got, want, tag, sl=slice(None)):
    for k in OUTPUTS:
        assert got[k].shape == want[k][:, :, sl].shape, (tag, k)
        err = _gap(got[k], want[k][:, :, sl])
        print("%s %s: max |session - Transfer| = %.3e" % (tag, k, err))
        assert err < FRAMES, (tag, k, err)
    assert set(got["kp_norm"]) == set(want["kp_norm"]) == {"mean", "var"}
    for k in want["kp_norm"]:
        err = _gap(got["kp_norm"][k], want["kp_norm"][k][:, sl])
        print("%s kp_norm[%s]: %.3e" % (tag, k, err))
        assert err < KP, (tag, k, err)
    for k in want["kp_source"]:
        assert torch.equal(got["kp_source"][k], want["kp_source"][k]), (tag, k)


@pytest.mark.parametrize("splits", [(1, 3, 1), (5,)], ids=["1+3+1", "5"])
def test_session_equals_the_whole_video_transfer(be, splits):
    from mnk import engine
    gen, kpd, src, driving, whole, size = _setup(be)
    s = engine.AnimationSession(kpd, gen, PARAMS)
    s.set_source(src)
    got = _pushes(s, driving, splits)
    be.sync()
    assert got["video_prediction"].shape == (2, 3, D, size, size) and s.frames_pushed == D
    _check(got, whole, "+".join(map(str, splits)))
    if len(splits) == 1:        # the same detector call, the same normalisation kernel, the same generator launches
        assert torch.equal(bits(got["kp_norm"]["mean"]), bits(whole["kp_norm"]["mean"]))
        assert torch.equal(bits(got["video_prediction"]), bits(whole["video_prediction"]))


def test_the_anchor_matters(be):
    """Transfer chunk by chunk anchors every chunk to its own first frame: its kp_norm leaves the whole video's by far more than
    rounding on a later chunk (the jump at a chunk boundary); the session's does not."""
    from mnk import engine
    gen, kpd, src, driving, whole, _ = _setup(be)
    transfer = engine.Transfer(kpd, gen, PARAMS, shared_source=True)
    s = engine.AnimationSession(kpd, gen, PARAMS)
    s.set_source(src)
    at, worst = 0, 0.0
    for n in (1, 3, 1):
        per_chunk = transfer(src, driving[:, :, at:at + n])
        pushed = s.push(driving[:, :, at:at + n])
        be.sync()
        want = whole["kp_norm"]["mean"][:, at:at + n]
        gap_t, gap_s = _gap(per_chunk["kp_norm"]["mean"], want), _gap(pushed["kp_norm"]["mean"], want)
        print("frames %d..%d: |Transfer per chunk - whole| = %.3e, |session - whole| = %.3e" % (at, at + n - 1, gap_t, gap_s))
        assert gap_s < KP
        if at > 0:
            worst = max(worst, gap_t)
            assert gap_t > 1e-3, (at, gap_t)
        at += n


def test_chunked_transfer_equals_the_unchunked_call(be):
    from mnk import engine
    gen, kpd, src, driving, whole, _ = _setup(be)
    got = engine.Transfer(kpd, gen, PARAMS, shared_source=True, chunk=2)(src, driving)       # 2 + 2 + 1
    be.sync()
    assert set(got) == set(whole)
    _check(got, whole, "chunk=2")
    for k in whole["kp_driving"]:
        assert _gap(got["kp_driving"][k], whole["kp_driving"][k]) < KP
    with pytest.raises(ValueError):
        engine.Transfer(kpd, gen, PARAMS, chunk=2)
    with pytest.raises(ValueError):
        engine.Transfer(kpd, gen, PARAMS, shared_source=True, chunk=0)


@pytest.mark.parametrize("d", [1, 3])
def test_generator_with_a_source_state_gives_the_same_bits(be, d):
    """only the encoder and the source conversions are skipped: the same launches follow"""
    gen, kpd, src, driving, whole, _ = _setup(be)
    kp_d = {k: v[:, :d].contiguous() for k, v in whole["kp_norm"].items()}
    kp_s = whole["kp_source"]
    with torch.no_grad():
        want = gen(src, kp_driving=kp_d, kp_source=kp_s)
        state = gen.encode_source(src)
        got = gen(src, kp_d, kp_s, source_state=state)
        again = gen(src, kp_d, kp_s, source_state=state)            # the state is read, not consumed
    be.sync()
    for k in OUTPUTS:
        assert torch.equal(bits(got[k]), bits(want[k])) and torch.equal(bits(again[k]), bits(want[k])), k
    assert (state.B, state.H, state.W) == (2, src.shape[3], src.shape[4])
    from mnk import ops
    assert ops.handover_state() == {}


def test_a_source_state_in_training_mode_raises(be):
    gen, kpd, src, driving, whole, _ = _setup(be)
    kp_d = {k: v[:, :1].contiguous() for k, v in whole["kp_norm"].items()}
    with torch.no_grad():
        state = gen.encode_source(src)
    gen.train()
    try:
        with pytest.raises(RuntimeError):
            gen(src, kp_d, whole["kp_source"], source_state=state)
        with pytest.raises(RuntimeError):
            gen.encode_source(src)
    finally:
        gen.eval()
    with torch.no_grad(), pytest.raises(ValueError):                 # a state of another batch size
        gen(src[:1], {k: v[:1] for k, v in kp_d.items()}, {k: v[:1] for k, v in whole["kp_source"].items()}, source_state=state)


@pytest.mark.parametrize("params", [None, dict(movement_mult=True, clip_mean=False)], ids=["None", "neither-option"])
def test_without_normalisation_the_session_is_the_reconstruction_loop(be, params):
    """reconstruction.py:12-25: the detector's key-points go to the generator as they are, no anchor is kept"""
    from mnk import engine
    gen, kpd, src, driving, _, _ = _setup(be)
    want = engine.Reconstructor(kpd, gen)(src, driving)
    s = engine.AnimationSession(kpd, gen, params)
    s.set_source(src)
    got = _pushes(s, driving, (2, 3))
    be.sync()
    for k in OUTPUTS:
        err = _gap(got[k], want[k])
        print("%s: max |session - Reconstructor| = %.3e" % (k, err))
        assert err < FRAMES, k
    for k in got["kp_driving"]:
        assert torch.equal(got["kp_norm"][k], got["kp_driving"][k])
    assert _gap(got["kp_driving"]["mean"], want["kp_driving_mean"]) < FRAMES
    assert not s.anchor.anchored


def test_reset_anchors_again_and_the_source_stays(be):
    from mnk import engine
    gen, kpd, src, driving, _, _ = _setup(be)
    s = engine.AnimationSession(kpd, gen, PARAMS)
    s.set_source(src)
    s.push(driving[:, :, 0:2])
    assert s.frames_pushed == 2 and s.anchor.anchored
    s.reset()
    assert s.frames_pushed == 0 and not s.anchor.anchored
    got = _pushes(s, driving[:, :, 2:], (1, 2))
    want = engine.Transfer(kpd, gen, PARAMS, shared_source=True)(src, driving[:, :, 2:])
    be.sync()
    _check(got, want, "after reset")


def test_a_second_source_of_the_same_shape_equals_a_fresh_session(be):
    from mnk import engine
    gen, kpd, src, driving, _, size = _setup(be)
    src2 = be.t(cases.smooth_pair(2, size, size, seed=12)[0])
    s = engine.AnimationSession(kpd, gen, PARAMS)
    s.set_source(src)
    s.push(driving[:, :, 0:2])
    state = s._state
    s.set_source(src2)                                               # in place: the cached tensors keep their storage
    assert s._state is state and s.frames_pushed == 0
    got = _pushes(s, driving, (2, 3))
    fresh = engine.AnimationSession(kpd, gen, PARAMS)
    fresh.set_source(src2)
    want = _pushes(fresh, driving, (2, 3))
    be.sync()
    for k in OUTPUTS:
        assert torch.equal(bits(got[k]), bits(want[k])), k
    for k in ("kp_norm", "kp_source", "kp_driving"):
        for kk in want[k]:
            assert torch.equal(bits(got[k][kk]), bits(want[k][kk])), (k, kk)
    assert not torch.equal(bits(got["kp_source"]["mean"]), bits(kpd(src)["mean"].detach()))


def test_error_cases(be):
    from mnk import engine
    gen, kpd, src, driving, _, size = _setup(be)
    s = engine.AnimationSession(kpd, gen, PARAMS)
    with pytest.raises(ValueError):
        s.push(driving[:, :, :1])                                    # before set_source
    with pytest.raises(ValueError):
        s.set_source(driving[:, :, :2])                              # two source frames
    s.set_source(src)
    for bad in (driving[:1, :, :1], driving[:, :2, :1], driving[:, :, :1, : size // 2], driving[:, :, :1, :, : size // 2],
                driving[:, :, :0], driving[:, :, 0]):
        with pytest.raises(ValueError):
            s.push(bad)
    assert s.frames_pushed == 0 and not s.anchor.anchored
    clip = engine.AnimationSession(kpd, gen, dict(clip_mean=True, adapt_variance=True))
    clip.set_source(src)
    with pytest.raises(NameError):
        clip.push(driving[:, :, :1])
    with pytest.raises(ValueError):
        engine.AnimationSession(kpd, gen, PARAMS, precision="fp16")
    # the anchored normalize_kp refuses an anchor of other key-points
    with torch.no_grad():
        kp_d, kp_s = kpd(driving[:, :, :2]), kpd(src)
        a = engine.KpAnchor()
        engine.normalize_kp(kp_d, kp_s, anchor=a, **PARAMS)
        with pytest.raises(ValueError):
            engine.normalize_kp({k: v[:1] for k, v in kp_d.items()}, {k: v[:1] for k, v in kp_s.items()}, anchor=a, **PARAMS)


def test_normalize_kp_with_an_anchor_equals_the_whole_call_bit_for_bit(be):
    from mnk import engine
    gen, kpd, src, driving, whole, _ = _setup(be)
    a = engine.KpAnchor()
    parts = [engine.normalize_kp({k: v[:, s:e].contiguous() for k, v in whole["kp_driving"].items()}, whole["kp_source"], anchor=a,
                                 **PARAMS) for s, e in ((0, 2), (2, 5))]
    be.sync()
    for k in ("mean", "var"):
        assert torch.equal(bits(torch.cat([p[k] for p in parts], dim=1)), bits(whole["kp_norm"][k])), k


def test_session_under_bf16_fused_skinny_options(be):
    """The session against Transfer(shared_source=True), both under precision="bf16", fuse_norm=True, skinny=True.  Bound: twice
    what Transfer whole-video shared-source and Transfer repeated-source show between them under the same options (measured
    here).  Those two run ONE detector call on all five frames, so the session case that is bounded is the one with that
    detector call, a push of five: a push of fewer frames re-batches the detector, whose fp32 rounding differences a bf16
    operand rounding downstream can turn into a bf16 ulp -- that figure is printed, not bounded by this pair."""
    from mnk import engine
    gen, kpd, src, driving, _, _ = _setup(be)
    opts = dict(precision="bf16", fuse_norm=True, skinny=True)
    shared = engine.Transfer(kpd, gen, PARAMS, shared_source=True, **opts)(src, driving)
    repeated = engine.Transfer(kpd, gen, PARAMS, **opts)(src, driving)
    s = engine.AnimationSession(kpd, gen, PARAMS, **opts)
    assert s.options == (("bf16", True, True))
    s.set_source(src)
    got = _pushes(s, driving, (5,))
    s.reset()
    split = _pushes(s, driving, (1, 3, 1))
    be.sync()
    for k in OUTPUTS:
        pair, err, err_split = _gap(shared[k], repeated[k]), _gap(got[k], shared[k]), _gap(split[k], shared[k])
        print("%s: |Transfer shared - repeated| = %.3e, |session(5) - Transfer shared| = %.3e, |session(1+3+1) - Transfer shared| "
              "= %.3e" % (k, pair, err, err_split))
        assert err <= 2 * pair, (k, err, pair)
    from mnk import ops
    assert ops.current_eval_options() == ops.EvalOptions() and ops.handover_state() == {}
