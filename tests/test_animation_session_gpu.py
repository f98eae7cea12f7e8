"""mnk.engine.AnimationSession with use_graph on the MI355X: one linear hipGraph per (B, n) push shape.  The captured program runs
the kernels of the eager push in the same order, so every push is bit-equal (the criterion of
test_hipgraph_replay_equals_eager_launches) -- the push that anchors, a push after reset(), a push after a same-shape
set_source() -- and a second push shape gets a program of its own that leaves the first one usable.  The programs hold frozen
weights: after load_state_dict + set_source() the next push runs on the new weights.  Tiny models, B = 2, n = 2."""
import pytest
import torch

from oracle import cases
from test_modules import load, build

PARAMS = dict(movement_mult=True, move_location=True, adapt_variance=True, clip_mean=True)


def _keep(out):
    """a captured push returns static buffers: clone what is compared later"""
    return {k: (v.clone() if torch.is_tensor(v) else {kk: t.clone() for kk, t in v.items()}) for k, v in out.items()}


def _same_bits(a, b, tag):
    for k in ("video_prediction", "video_deformed"):
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (tag, k)
    for k in ("kp_driving", "kp_source", "kp_norm"):
        for kk in a[k]:
            assert torch.equal(a[k][kk].contiguous().view(torch.int32), b[k][kk].contiguous().view(torch.int32)), (tag, k, kk)


@pytest.mark.gpu
def test_captured_session_equals_the_eager_session_bit_for_bit():
    from conftest import Backend
    from mnk import engine
    be = Backend("hip")
    gold = load("tiny")
    gen, _, kpd = build(gold["cfg"])
    gen.load_state_dict(gold["state"]["generator"]), kpd.load_state_dict(gold["state"]["kp_detector"])
    gen.to(be.device).eval(), kpd.to(be.device).eval()
    size = gold["size"]
    src = be.t(cases.smooth_pair(2, size, size, seed=11)[0])
    src2 = be.t(cases.smooth_pair(2, size, size, seed=12)[0])
    driving = be.t(torch.cat([cases.smooth_pair(2, size, size, seed=20 + i)[1] for i in range(6)], dim=2))
    eager = engine.AnimationSession(kpd, gen, PARAMS, use_graph=False)
    graphed = engine.AnimationSession(kpd, gen, PARAMS, use_graph=True)
    both = (eager, graphed)

    def push(lo, hi, tag):
        a, b = eager.push(driving[:, :, lo:hi]), _keep(graphed.push(driving[:, :, lo:hi]))
        torch.cuda.synchronize()
        _same_bits(a, b, tag)
        return b

    for s in both:
        s.set_source(src)
    first = push(0, 2, "the push that anchors (and captures: the warm-up pushes must not leave their anchor)")
    assert graphed.anchor.anchored and list(graphed._programs) == [(2, 2)]
    push(2, 4, "a later push")
    later = push(4, 6, "a third push")
    assert eager.frames_pushed == graphed.frames_pushed == 6
    for s in both:
        s.reset()
    after_reset = push(4, 6, "the push after reset() anchors again")
    assert not torch.equal(after_reset["kp_norm"]["mean"], later["kp_norm"]["mean"])         # another anchor, other key-points
    for s in both:
        s.set_source(src2)
    push(2, 4, "the push after a same-shape set_source()")
    assert list(graphed._programs) == [(2, 2)]                                               # written in place: no new program
    push(0, 1, "a second push shape, captured while an anchor is held")
    assert sorted(graphed._programs) == [(2, 1), (2, 2)]
    push(4, 6, "the first program after the second one")
    # from a fresh anchor the first program gives the first push's key-points for the first source again
    for s in both:
        s.set_source(src)
    again = push(0, 2, "the first program, first source, fresh anchor")
    _same_bits(again, first, "replay of the first push")
    # other weights: the programs were captured with frozen weights and must follow them (set_source re-encodes the source)
    sd = {k: v.detach().cpu().clone() for k, v in gen.state_dict().items()}
    cases.perturb_state_dict(sd, 31)
    gen.load_state_dict(sd)
    for s in both:
        s.set_source(src)
    other = push(0, 2, "after load_state_dict + set_source()")
    assert not torch.equal(other["video_prediction"], first["video_prediction"])
    push(2, 4, "a later push on the new weights")
