"""uint8 frames in and out of AnimationSession, Transfer, Reconstructor and the modules (ops.U8Frames, output="uint8").

The `tiny` golden's models and the inputs of test_animation_session.py (B = 2, five driving frames, all four normalisation
options), quantised ONCE to uint8 channel-last -- what a decoder hands over (frames_dataset.py:14-40).  The fp32 comparison input is
U8Frames(...).float(): `img_as_float32` of the same bytes.  Every comparison is exact: a uint8 input reaches the same act as that
fp32 tensor (tests/test_kernels_u8_frames.py) and the same launches follow; a uint8 output is the same kernel's value through
`(255 * x).astype(np.uint8)`."""
import copy

import pytest
import torch

from oracle import cases
from test_animation_session import _setup, _keep, bits, PARAMS, D, OUTPUTS

SPLITS = [(1, 3, 1), (5,)]
IDS = ["1+3+1", "5"]


def quantise(t):
    """(B, C, n, H, W) in [0, 1] -> uint8 (B, n, H, W, C)"""
    return (t.detach().cpu() * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()


_U8 = {}


def _inputs(be):
    """models and the quantised inputs: uint8 (device), their fp32 tensors; made once per backend, never written to"""
    if be.kind not in _U8:
        from mnk import ops
        gen, kpd, src, driving, _, size = _setup(be)
        src8, drv8 = be.t(quantise(src)), be.t(quantise(driving))
        _U8[be.kind] = dict(gen=gen, kpd=kpd, size=size, src8=src8, drv8=drv8, src=ops.U8Frames(src8).float(),
                            drv=ops.U8Frames(drv8).float(), runs={})
    return _U8[be.kind]


def _pushes(session, frames, splits, fdim=2):
    """frames: a float (B, C, n, H, W) tensor, a U8Frames, or a uint8 (B, n, H, W, C) tensor; fdim: the outputs' frame axis"""
    parts, at = [], 0
    for n in splits:
        chunk = frames[:, at:at + n] if torch.is_tensor(frames) and frames.dtype == torch.uint8 else frames[:, :, at:at + n]
        parts.append(_keep(session.push(chunk)))
        at += n
    assert at == D
    return {"video_prediction": torch.cat([p["video_prediction"] for p in parts], dim=fdim),
            "video_deformed": torch.cat([p["video_deformed"] for p in parts], dim=fdim),
            "kp_driving": {k: torch.cat([p["kp_driving"][k] for p in parts], dim=1) for k in parts[0]["kp_driving"]},
            "kp_norm": {k: torch.cat([p["kp_norm"][k] for p in parts], dim=1) for k in parts[0]["kp_norm"]},
            "kp_source": parts[0]["kp_source"]}


def _float_run(be, splits):
    """the session fed the fp32 tensors, float output: the reference of every comparison here (once per backend and split)"""
    from mnk import engine
    u = _inputs(be)
    if splits not in u["runs"]:
        s = engine.AnimationSession(u["kpd"], u["gen"], PARAMS)
        s.set_source(u["src"])
        u["runs"][splits] = _pushes(s, u["drv"], splits)
        be.sync()
    return u["runs"][splits]


def _same_bits(got, want, tag, videos=True):
    for k in (OUTPUTS if videos else ()):
        assert got[k].dtype == want[k].dtype and torch.equal(bits(got[k]), bits(want[k])), (tag, k)
    for k in ("kp_driving", "kp_norm", "kp_source"):
        assert set(got[k]) == set(want[k])
        for kk in want[k]:
            assert torch.equal(bits(got[k][kk]), bits(want[k][kk])), (tag, k, kk)


def _as_bytes(video):
    """`(255 * out).astype(np.uint8)` on (..., H, W, C) (demo.py:69-71)"""
    return (255 * video.cpu()).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()


def _same_bytes(got, want, tag):
    u8 = (got["video_prediction"].dtype, got["video_deformed"].dtype)
    assert u8 == (torch.uint8, torch.uint8), (tag, u8)
    for k in OUTPUTS:
        w = _as_bytes(want[k])
        assert got[k].shape == w.shape and torch.equal(got[k].cpu(), w), (tag, k)
    _same_bits(got, want, tag, videos=False)


# ---- the session -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", SPLITS, ids=IDS)
def test_session_fed_uint8_equals_the_session_fed_float_bit_for_bit(be, splits):
    from mnk import engine, ops
    u, want = _inputs(be), _float_run(be, splits)
    wrap = ops.U8Frames if len(splits) == 1 else (lambda t: t)       # a U8Frames; the bare uint8 tensor
    s = engine.AnimationSession(u["kpd"], u["gen"], PARAMS)
    s.set_source(wrap(u["src8"]))
    assert ops.is_u8(s._source) and s._source.data.dtype == torch.uint8          # no fp32 copy of the source is kept
    got = _pushes(s, wrap(u["drv8"]), splits)
    be.sync()
    assert got["video_prediction"].shape == (2, 3, D, u["size"], u["size"]) and s.frames_pushed == D
    _same_bits(got, want, "+".join(map(str, splits)))


@pytest.mark.parametrize("splits", SPLITS, ids=IDS)
def test_uint8_output_is_the_float_output_through_255x_astype_uint8(be, splits):
    from mnk import engine
    u, want = _inputs(be), _float_run(be, splits)
    s = engine.AnimationSession(u["kpd"], u["gen"], PARAMS, output="uint8")
    s.set_source(u["src8"])
    got = _pushes(s, u["drv8"], splits, fdim=1)
    be.sync()
    assert got["video_prediction"].shape == (2, D, u["size"], u["size"], 3)
    _same_bytes(got, want, "u8 in, u8 out")
    assert len(torch.unique(got["video_prediction"])) > 2           # (frames, not a constant)
    f = engine.AnimationSession(u["kpd"], u["gen"], PARAMS, output="uint8")      # float frames in, uint8 frames out
    f.set_source(u["src"])
    _same_bytes(_pushes(f, u["drv"], splits, fdim=1), want, "float in, u8 out")


@pytest.mark.parametrize("cs", [1, 4])
def test_gray_and_rgba_inputs_equal_the_rgb_input_made_from_them(be, cs):
    from mnk import engine, ops
    u = _inputs(be)
    if cs == 1:
        src8, drv8 = u["src8"][..., 1:2].contiguous(), u["drv8"][..., 1:2].contiguous()
        rgb = lambda t: t.expand(-1, -1, -1, -1, 3).contiguous()                     # gray2rgb (frames_dataset.py:18-19)
    else:
        alpha = lambda t: ((t[..., :1].to(torch.int32) * 7 + 13) % 256).to(torch.uint8)
        src8, drv8 = torch.cat([u["src8"], alpha(u["src8"])], dim=-1), torch.cat([u["drv8"], alpha(u["drv8"])], dim=-1)
        rgb = lambda t: t[..., :3].contiguous()                                      # alpha dropped (:21-22)
    assert tuple(ops.U8Frames(src8).shape) == (2, 3, 1, u["size"], u["size"])
    assert torch.equal(ops.U8Frames(src8).float(), ops.U8Frames(rgb(src8)).float())
    outs = []
    for a, b in ((src8, drv8), (rgb(src8), rgb(drv8))):
        s = engine.AnimationSession(u["kpd"], u["gen"], PARAMS, output="uint8")
        s.set_source(a)
        outs.append(_pushes(s, b, (2, 3), fdim=1))
    be.sync()
    for k in OUTPUTS:
        assert torch.equal(outs[0][k], outs[1][k]), k
    _same_bits(outs[0], outs[1], "Cs = %d" % cs, videos=False)


def test_a_second_uint8_source_of_the_same_shape_is_written_in_place(be):
    from mnk import engine
    u = _inputs(be)
    src2 = be.t(quantise(cases.smooth_pair(2, u["size"], u["size"], seed=12)[0]))
    s = engine.AnimationSession(u["kpd"], u["gen"], PARAMS)
    s.set_source(u["src8"])
    s.push(u["drv8"][:, :2])
    state, kept = s._state, s._source
    s.set_source(src2)
    assert s._state is state and s._source is kept and torch.equal(kept.data, src2) and s.frames_pushed == 0
    got = _pushes(s, u["drv8"], (2, 3))
    fresh = engine.AnimationSession(u["kpd"], u["gen"], PARAMS)
    fresh.set_source(src2)
    _same_bits(got, _pushes(fresh, u["drv8"], (2, 3)), "second source")
    s.set_source(u["src"])                                           # another input kind: a new state
    assert s._state is not state and not torch.is_tensor(kept) and torch.is_tensor(s._source)


# ---- Transfer, Reconstructor -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "repeated"])
def test_transfer_takes_uint8_frames_and_returns_them(be, shared):
    from mnk import engine, ops
    u = _inputs(be)
    want = engine.Transfer(u["kpd"], u["gen"], PARAMS, shared_source=shared)(u["src"], u["drv"])
    src, drv = (ops.U8Frames(u["src8"]), u["drv8"]) if shared else (u["src8"], ops.U8Frames(u["drv8"]))
    got = engine.Transfer(u["kpd"], u["gen"], PARAMS, shared_source=shared)(src, drv)
    be.sync()
    _same_bits(got, want, "Transfer")
    got = engine.Transfer(u["kpd"], u["gen"], PARAMS, shared_source=shared, output="uint8")(u["src8"], u["drv8"])
    be.sync()
    _same_bytes(got, want, "Transfer u8")
    if shared:
        chunked = engine.Transfer(u["kpd"], u["gen"], PARAMS, shared_source=True, chunk=2, output="uint8")(u["src8"], u["drv8"])
        assert chunked["video_prediction"].shape == got["video_prediction"].shape
        assert chunked["video_prediction"].dtype == torch.uint8
        # (pushes of 2 + 2 + 1 re-batch the detector: the frames agree to the session's bound of 2e-6, one byte step at an edge)
        gap = (chunked["video_prediction"].cpu().int() - got["video_prediction"].cpu().int()).abs().max()
        assert int(gap) <= 1


def test_reconstructor_takes_uint8_frames_and_returns_them(be):
    from mnk import engine, ops
    u = _inputs(be)
    want = engine.Reconstructor(u["kpd"], u["gen"])(u["src"], u["drv"])
    got = engine.Reconstructor(u["kpd"], u["gen"])(ops.U8Frames(u["src8"]), u["drv8"])
    out8 = engine.Reconstructor(u["kpd"], u["gen"], output="uint8")(u["src8"], u["drv8"])
    be.sync()
    for k in OUTPUTS:
        assert torch.equal(bits(got[k]), bits(want[k])), k
        assert out8[k].dtype == torch.uint8 and torch.equal(out8[k].cpu(), _as_bytes(want[k])), k
    for k in ("kp_driving_mean", "kp_source_mean"):
        assert torch.equal(bits(got[k]), bits(want[k])) and torch.equal(bits(out8[k]), bits(want[k])), k


# ---- the modules -------------------------------------------------------------------------------------------------------------------
def _variant(mask_on, emb_on):
    cfg = copy.deepcopy(cases.TINY)
    gp = cfg["model_params"]["generator_params"]
    gp["dense_motion_params"]["mask_embedding_params"]["use_deformed_source_image"] = mask_on
    gp["kp_embedding_params"]["use_deformed_source_image"] = emb_on
    return cfg


@pytest.mark.parametrize("mask_on,emb_on", [(True, False), (False, True)], ids=["mask", "embedding"])
def test_modules_take_a_uint8_source_with_and_without_the_deformed_source_image(be, mask_on, emb_on):
    """oracle.cases.TINY with use_deformed_source_image on / off in the mask embedding and in the key-point embedding: the forward
    and encode_source on a uint8 source equal those on its fp32 tensor, bit for bit"""
    from mnk import ops
    from test_modules import build
    u = _inputs(be)
    gen, _, kpd = build(_variant(mask_on, emb_on))
    for i, m in enumerate((gen, kpd)):
        sd = m.state_dict()
        cases.perturb_state_dict(sd, 31 + i)
        m.load_state_dict(sd)
        m.to(be.device).eval()
    src8, drv8 = ops.U8Frames(u["src8"]), ops.U8Frames(u["drv8"][:, :2].contiguous())
    with torch.no_grad():
        kp_s, kp_d = kpd(src8), kpd(drv8)
        for k in kp_s:
            assert torch.equal(bits(kp_s[k]), bits(kpd(src8.float())[k])) and torch.equal(bits(kp_d[k]), bits(kpd(drv8.float())[k]))
        want = gen(src8.float(), kp_d, kp_s)
        state = gen.encode_source(src8)
        assert (state.mask_src is not None) == mask_on and (state.emb_src is not None) == emb_on
        runs = {"forward": gen(src8, kp_d, kp_s), "state": gen(src8, kp_d, kp_s, source_state=state),
                "float state": gen(src8, kp_d, kp_s, source_state=gen.encode_source(src8.float()))}
        out8 = gen(src8, kp_d, kp_s, source_state=state, output="uint8")
    be.sync()
    for tag, got in runs.items():
        for k in OUTPUTS:
            assert torch.equal(bits(got[k]), bits(want[k])), (tag, k)
    for k in OUTPUTS:
        assert torch.equal(out8[k].cpu(), _as_bytes(want[k])), k
    assert ops.handover_state() == {}


def test_u8frames_presents_the_float_tensor_without_its_values(be):
    from mnk import ops
    u = _inputs(be)
    f = ops.U8Frames(u["drv8"])
    assert tuple(f.shape) == (2, 3, D, u["size"], u["size"]) and f.dim() == 5 and f.device == u["drv8"].device
    assert f.type() == u["drv"].type() and f.float().dtype == torch.float32 and f.float().shape == f.shape
    want = u["drv8"].cpu().permute(0, 4, 1, 2, 3).float() * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    assert torch.equal(bits(f.float()), bits(want))
    assert torch.equal(f[:, :, 1:3].data, u["drv8"][:, 1:3]) and tuple(f[:1].shape) == (1, 3, D, u["size"], u["size"])
    for step in (1, 2):
        assert torch.equal(bits(ops.to_act(f, step)), bits(ops.to_act(f.float(), step)))


class _Recorder:
    def __init__(self, monkeypatch):
        from mnk import ops
        self.names, inner = [], ops._call

        def call(name, ref, *args):
            self.names.append(name)
            return inner(name, ref, *args)
        monkeypatch.setattr(ops, "_call", call)


def test_a_uint8_push_issues_no_float_frame_conversion(be, monkeypatch):
    from mnk import engine
    u = _inputs(be)
    rec = _Recorder(monkeypatch)
    s = engine.AnimationSession(u["kpd"], u["gen"], PARAMS, use_graph=False, output="uint8")
    s.set_source(u["src8"])
    setup = list(rec.names)
    del rec.names[:]
    s.push(u["drv8"][:, :2])
    be.sync()
    banned = {"mnk_ncdhw_to_nhwc", "mnk_nhwc_to_ncdhw", "mnk_nhwc_to_ncdhw_strided", "mnk_frames_to_strip", "mnk_conv1x1_fwd"}
    assert not banned & set(setup) and not banned & set(rec.names), sorted(banned & set(setup + rec.names))
    assert rec.names.count("mnk_u8_to_nhwc") == 1 and rec.names.count("mnk_conv1x1_fwd_u8") == 1       # the detector's input; conv-last
    assert rec.names.count("mnk_nhwc_to_u8") == 1 and "mnk_u8_to_nhwc" in setup
    del rec.names[:]                                                 # the float path of the same build still converts
    f = engine.AnimationSession(u["kpd"], u["gen"], PARAMS, use_graph=False)
    f.set_source(u["src"])
    f.push(u["drv"][:, :, :2])
    assert {"mnk_ncdhw_to_nhwc", "mnk_nhwc_to_ncdhw", "mnk_conv1x1_fwd"} <= set(rec.names) and "mnk_u8_to_nhwc" not in rec.names


def test_errors_name_the_fix(be):
    from mnk import engine, ops
    u = _inputs(be)
    gen, kpd, size = u["gen"], u["kpd"], u["size"]
    src8, drv8 = ops.U8Frames(u["src8"]), ops.U8Frames(u["drv8"][:, :1].contiguous())
    with torch.no_grad():
        kp_s, kp_d = kpd(src8), kpd(drv8)
    for m, call in ((kpd, lambda: kpd(src8)), (gen, lambda: gen(src8, kp_d, kp_s)), (gen, lambda: gen.encode_source(src8))):
        m.train()
        try:
            with torch.no_grad(), pytest.raises(RuntimeError, match="eval"):                 # uint8 input in training mode
                call()
        finally:
            m.eval()
    assert any(p.requires_grad for p in kpd.parameters())
    with pytest.raises(RuntimeError, match="no_grad"):                                       # ... with grad on a trainable model
        kpd(src8)
    with pytest.raises(RuntimeError, match="no_grad"):
        gen(src8, kp_d, kp_s)
    with pytest.raises(RuntimeError, match="no_grad"):                                       # uint8 output outside no_grad
        gen(src8.float(), kp_d, kp_s, output="uint8")
    gen.train()
    try:
        with torch.no_grad(), pytest.raises(RuntimeError, match="eval"):                     # ... outside evaluation mode
            gen(src8.float(), kp_d, kp_s, output="uint8")
    finally:
        gen.eval()
    s = engine.AnimationSession(kpd, gen, PARAMS)
    s.set_source(u["src8"])
    zeros = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=be.device)
    with pytest.raises(ValueError, match="C = 1"):                                           # Cs = 2
        s.push(zeros(2, 1, size, size, 2))
    with pytest.raises(ValueError, match="channel-last"):                                    # a 4-d uint8 tensor
        s.push(zeros(2, size, size, 3))
    with pytest.raises(ValueError, match="channel-last"):
        s.set_source(zeros(2, size, size, 3))
    with pytest.raises(ValueError, match="differ from the source"):                          # another frame size
        s.push(zeros(2, 1, size // 2, size, 3))
    with pytest.raises(ValueError, match="differ from the source"):
        s.push(zeros(1, 1, size, size, 3))
    assert s.frames_pushed == 0
    for make in (lambda: engine.AnimationSession(kpd, gen, PARAMS, output="bytes"),
                 lambda: engine.Transfer(kpd, gen, PARAMS, output="u8"), lambda: engine.Reconstructor(kpd, gen, output=None)):
        with pytest.raises(ValueError, match='"uint8"'):                                     # an unknown output
            make()
    with torch.no_grad(), pytest.raises(ValueError, match='"uint8"'):
        gen(src8, kp_d, kp_s, output="byte")
    with pytest.raises(ValueError, match="uint8"):
        ops.U8Frames(u["drv"])


# ---- the captured push (device build) ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("output", ["float", "uint8"])
def test_captured_uint8_push_equals_the_eager_push(make_backend, output):
    from mnk import engine
    be = make_backend("hip")
    u = _inputs(be)
    fdim = 1 if output == "uint8" else 2
    runs = {}
    for graph in (True, False):
        s = engine.AnimationSession(u["kpd"], u["gen"], PARAMS, use_graph=graph, output=output)
        s.set_source(u["src8"])
        runs[graph] = _pushes(s, u["drv8"], (1, 3, 1), fdim=fdim)
        if graph:
            assert len(s._programs) == 2 and all(k[2] == ("uint8", 3) and k[3] == output for k in s._programs)
            for prog in s._programs.values():
                assert prog[1].data.dtype == torch.uint8 and prog[1].data.is_cuda            # the static input is the byte buffer
                assert prog[2]["video_prediction"].dtype == (torch.uint8 if output == "uint8" else torch.float32)
        else:
            assert not s._programs
    be.sync()
    for k in OUTPUTS:
        assert torch.equal(runs[True][k], runs[False][k]), k
    _same_bits(runs[True], runs[False], "captured", videos=False)
    if output == "uint8":
        _same_bytes(runs[True], _float_run(be, (1, 3, 1)), "captured u8")


@pytest.mark.gpu
def test_captured_program_survives_a_second_source_and_takes_host_frames(make_backend):
    from mnk import engine
    be = make_backend("hip")
    u = _inputs(be)
    src2 = be.t(quantise(cases.smooth_pair(2, u["size"], u["size"], seed=12)[0]))
    s = engine.AnimationSession(u["kpd"], u["gen"], PARAMS, output="uint8")
    s.set_source(u["src8"])
    first = _keep(s.push(u["drv8"][:, :2]))
    progs = dict(s._programs)
    assert len(progs) == 1
    s.set_source(src2)                                               # same shape and kind: written in place, no re-capture
    got = _keep(s.push(u["drv8"][:, :2]))
    assert len(s._programs) == 1 and all(s._programs[k] is v for k, v in progs.items())
    fresh = engine.AnimationSession(u["kpd"], u["gen"], PARAMS, use_graph=False, output="uint8")
    fresh.set_source(src2)
    want = _keep(fresh.push(u["drv8"][:, :2]))
    be.sync()
    assert not torch.equal(got["video_prediction"], first["video_prediction"])
    for k in OUTPUTS:
        assert torch.equal(got[k], want[k]), k
    # host-resident bytes, pinned or not, captured and eager: one H2D copy of the bytes, the same frames
    host = u["drv8"][:, :2].cpu()
    for frames in (host, host.pin_memory()):
        for session in (s, fresh):
            session.reset()
            out = _keep(session.push(frames))
            be.sync()
            for k in OUTPUTS:
                assert out[k].is_cuda and torch.equal(out[k], want[k]), k
    assert len(s._programs) == 1
    hs = engine.AnimationSession(u["kpd"], u["gen"], PARAMS, use_graph=False, output="uint8")
    hs.set_source(src2.cpu())                                        # a host-resident source
    out = hs.push(host)
    be.sync()
    for k in OUTPUTS:
        assert torch.equal(out[k], want[k]), k
