"""torch.autograd wrappers around the C-ABI kernels of libmonkeynet_hip.so.

Internal activation format ("act"): a contiguous fp32 tensor of shape (N, H, W, ld) -- NHWC with the reference's
time axis D folded into N (frame = b*D + d) and the channel stride `ld` rounded up to a multiple of 4 (pad channels
are zero).  The logical channel count travels next to the tensor.  PyTorch is used for memory, streams and the
autograd tape only; every arithmetic step is a kernel launch through `mnk._lib` (no CPU / eager fallback).
"""
import weakref
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from . import knobs
from . import dist as mdist


def ceil4(c):
    return (c + 3) // 4 * 4


def ceil16(c):
    return (c + 15) // 16 * 16


def _p(t):
    return None if t is None else t.data_ptr()


# (the raw handle of the current stream without a torch.cuda.Stream object: 0.3 instead of 5 us per kernel launch -- the
# reference's own loop on these modules is bound by the host, not by the GPU: tools/dropin_profile.py)
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t):
    if not t.is_cuda:
        return 0
    if _RAW_STREAM is not None:
        return _RAW_STREAM(t.device.index)
    return torch.cuda.current_stream(t.device).cuda_stream


def _check_device(t):
    if not t.is_cuda and _lib.lib().is_device_build:
        raise _lib.MnkError("the MI355X hot path needs CUDA/HIP tensors; got a %s tensor (there is no CPU fallback)"
                            % t.device)


class _Scratch:
    """Grow-only scratch buffers, one per (purpose, device, stream): reuse between consecutive kernels of a stream is
    ordered by that stream, and a branch of work on a second stream gets buffers of its own."""

    def __init__(self):
        self.bufs = {}

    def get(self, key, nfloats, like):
        nfloats = max(int(nfloats), 1)
        k = (key, like.device, _stream(like))
        buf = self.bufs.get(k)
        if buf is None or buf.numel() < nfloats:
            buf = torch.empty(int(nfloats * 1.25) + 1024, dtype=torch.float32, device=like.device)
            self.bufs[k] = buf
        return buf


SCRATCH = _Scratch()


def _call(name, ref, *args):
    _lib.lib().call(name, *args, _stream(ref))


def _query(name, *args):
    return _lib.lib().query(name, *args)


class _EvalCtx:
    """What a Function.forward of this module sees as `ctx` when it runs OUTSIDE autograd (grad mode off): nothing is saved,
    no input needs a gradient; attributes a forward sets (ctx.meta = ...) land on this throw-away object."""
    __slots__ = ("__dict__", "needs_input_grad")

    def __init__(self, n):
        self.needs_input_grad = (False,) * n

    def save_for_backward(self, *tensors):
        pass

    def mark_non_differentiable(self, *tensors):
        pass

    def set_materialize_grads(self, value):
        pass


class _Fn(torch.autograd.Function):
    """torch.autograd.Function whose apply() calls forward() directly when grad mode is off: the evaluation loops of the
    reference (reconstruction.py:52-62, transfer.py:65-79, demo.py) run the networks frame by frame at batch 1 under
    torch.no_grad(), ~95 Function calls per frame, and are bound by the host (tools/frame_loop_probe.py) -- the autograd
    machinery of apply() (argument scan, node construction, output wrapping) has nothing to record there."""

    @classmethod
    def apply(cls, *args):
        if torch.is_grad_enabled():
            return super().apply(*args)
        return cls.forward(_EvalCtx(len(args)), *args)


# ----------------------------------------------------------------------------------------------------------------
# layout
# ----------------------------------------------------------------------------------------------------------------
class ToActFn(_Fn):
    """(B,C,D,H,W) -> act, with the nearest down-scaling by an integer `step` (keypoint_detector.py:98-99)."""

    @staticmethod
    def forward(ctx, x5, step):
        _check_device(x5)
        x5 = x5.contiguous().float()
        b, c, d, h, w = x5.shape
        out = torch.empty(b * d, h // step, w // step, ceil4(c), dtype=torch.float32, device=x5.device)
        _call("mnk_ncdhw_to_nhwc", x5, _p(x5), _p(out), b, c, d, h, w, step, ceil4(c))
        ctx.meta = (b, c, d, h, w, step)
        return out

    @staticmethod
    def backward(ctx, g):
        b, c, d, h, w, step = ctx.meta
        g = g.contiguous()
        out = torch.empty(b, c, d, h, w, dtype=torch.float32, device=g.device)
        if step != 1:     # the nearest down-scaling picks x[..., ::step, ::step]: its adjoint fills the other pixels with 0
            _call("mnk_nhwc_to_ncdhw_strided", g, _p(g), g.shape[-1], _p(out), b, c, d, h, w, step)
        else:
            _call("mnk_nhwc_to_ncdhw", g, _p(g), g.shape[-1], _p(out), b, c, d, h, w)
        return out, None


class StackedBatch:
    """[a ; b] along the batch axis of two (B,C,D,H,W) tensors WITHOUT the concatenation: the only consumer of such a stack in
    the training iteration is the conversion to the kernels' layout (train.py:27 / :43-45 -> to_act), which writes the two
    halves of one act itself (ToActPairFn) -- torch.cat of contiguous tensors along dim 0 is two device-to-device memcpy
    launches in front of that conversion."""

    def __init__(self, a, b):
        assert a.shape == b.shape and a.dim() == 5
        self.parts = (a, b)
        self.shape = torch.Size((a.shape[0] + b.shape[0],) + tuple(a.shape[1:]))
        self.device = a.device

    def __getitem__(self, idx):
        b = self.parts[0].shape[0]
        if isinstance(idx, slice) and idx.start in (None, 0) and idx.step is None and idx.stop == b:
            return self.parts[0]
        return torch.cat(self.parts, dim=0)[idx]


OUTPUT_KINDS = ("float", "uint8")


def check_output(output):
    if output not in OUTPUT_KINDS:
        raise ValueError('output must be "float" (fp32 (B, C, d, H, W), the default) or "uint8" (channel-last (B, d, H, W, C) '
                         'frames); got %r' % (output,))
    return output


class U8Frames:
    """uint8 channel-last frames (B, n, H, W, Cs) -- what imageio, a decoder or a camera hand over (frames_dataset.py:14-40
    read_video) -- standing where the modules take the fp32 (B, 3, n, H, W) tensor of `img_as_float32` of them: gray (Cs = 1) is
    replicated to RGB, alpha (Cs = 4) is dropped.  It presents that tensor's shape, dim(), device and type(); the only consumer of
    its values is to_act, which converts the bytes straight into the kernels' layout (mnk_u8_to_nhwc): no fp32 copy of the frames
    exists.  Inference only: the modules refuse it in training mode, and under grad mode when a parameter requires grad.
    float(): the fp32 (B, 3, n, H, W) tensor of the same values (comparison paths, callers that need the tensor)."""

    def __init__(self, data):
        if not torch.is_tensor(data) or data.dtype != torch.uint8:
            raise ValueError("U8Frames takes a torch.uint8 tensor (B, n, H, W, C); got %s"
                             % (data.dtype if torch.is_tensor(data) else type(data).__name__,))
        if data.dim() != 5:
            raise ValueError("uint8 frames are channel-last (B, n, H, W, C) -- add the batch / frame axes with [None]; got %d-d %s"
                             % (data.dim(), tuple(data.shape)))
        if data.shape[4] not in (1, 3, 4):
            raise ValueError("uint8 frames have C = 1 (gray), 3 (RGB) or 4 (RGBA) channels in the LAST axis; got %s -- a channel-"
                             "first array needs .permute(0, 2, 3, 4, 1) first" % (tuple(data.shape),))
        self.data = data.contiguous()
        b, n, h, w, _ = data.shape
        self.shape = torch.Size((b, 3, n, h, w))

    device = property(lambda self: self.data.device)
    channels = property(lambda self: self.data.shape[4])
    kind = property(lambda self: ("uint8", self.data.shape[4]))

    def dim(self):
        return 5

    def size(self, i=None):
        return self.shape if i is None else self.shape[i]

    def type(self):
        return "torch.cuda.FloatTensor" if self.data.is_cuda else "torch.FloatTensor"

    def detach(self):
        return self

    def contiguous(self):
        return self

    def clone(self):
        return U8Frames(self.data.clone())

    def to(self, device, non_blocking=False):
        return self if self.data.device == torch.device(device) else U8Frames(self.data.to(device, non_blocking=non_blocking))

    def copy_(self, other, non_blocking=False):
        self.data.copy_(other.data, non_blocking=non_blocking)
        return self

    def repeat_interleave(self, repeats, dim=0):
        if dim != 0:
            raise NotImplementedError("U8Frames repeats along the batch axis only")
        return U8Frames(self.data.repeat_interleave(repeats, dim=0))

    def __getitem__(self, idx):
        """frames[:, :, i:j] (and batch slices): the same frames of the (B, 3, n, H, W) view, still as bytes"""
        idx = idx if isinstance(idx, tuple) else (idx,)
        if len(idx) > 3 or not all(isinstance(i, slice) for i in idx) or (len(idx) > 1 and idx[1] != slice(None)):
            raise NotImplementedError("U8Frames takes slices of the batch and the frame axis: frames[b0:b1, :, f0:f1]")
        data = self.data[idx[0]]
        return U8Frames(data[:, idx[2]] if len(idx) == 3 else data)

    def float(self):
        rgb = self.data.expand(-1, -1, -1, -1, 3) if self.data.shape[4] == 1 else self.data[..., :3]
        # img_as_float32: uint8 * float32(1 / 255), one fp32 product per value
        return (rgb.permute(0, 4, 1, 2, 3).float() * torch.tensor(1.0 / 255.0, dtype=torch.float32, device=rgb.device)).contiguous()


def is_u8(x):
    return isinstance(x, U8Frames)


def frame_kind(x):
    """what a captured program's static input is keyed by"""
    return x.kind if isinstance(x, U8Frames) else ("float", x.shape[1])


def as_frames(x, device=None):
    """What the engines take as frames: a float (B, C, n, H, W) tensor (as it is), a U8Frames, or a bare 5-d torch.uint8 tensor,
    which is taken as channel-last frames (B, n, H, W, C) and wrapped.  device: uint8 frames that live elsewhere (the host, pinned
    or not) are copied there -- the bytes, once."""
    if torch.is_tensor(x) and x.dtype == torch.uint8:
        x = U8Frames(x)
    if isinstance(x, U8Frames) and device is not None:
        x = x.to(device, non_blocking=True)
    return x


def module_device(module):
    """where a module's parameters live (None for a module without any): where host-resident uint8 frames are copied to"""
    p = next(module.parameters(), None)
    return None if p is None else p.device


def require_inference(module, x, what="uint8 frames"):
    """uint8 frames (and uint8 outputs) carry no gradient: evaluation mode, and no grad mode while a parameter requires grad"""
    if module.training:
        raise RuntimeError("%s serve inference only and %s is in training mode: call .eval() first (or pass the fp32 tensor, "
                           "U8Frames.float())" % (what, type(module).__name__))
    if torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters()):
        raise RuntimeError("%s serve inference only and %s has parameters that require grad under an enabled grad mode: wrap the "
                           "call in torch.no_grad() (or pass the fp32 tensor, U8Frames.float())" % (what, type(module).__name__))


def u8_to_act(x, step=1):
    """U8Frames -> act, with the nearest down-scaling by `step`: bit for bit ToActFn of x.float(), pad lanes included"""
    data = x.data
    _check_device(data)
    b, n, h, w, cs = data.shape
    out = torch.empty(b * n, h // step, w // step, 4, dtype=torch.float32, device=data.device)
    _call("mnk_u8_to_nhwc", data, _p(data), _p(out), b, n, h, w, cs, int(step), 4)
    return out


def act_to_u8(a, c, b):
    """act -> uint8 (B, d, H, W, C) = `(255 * from_act(a, c, b)).to(uint8)` channel-last (demo.py:69-71)"""
    _check_device(a)
    n, h, w, ld = a.shape
    out = torch.empty(b, n // b, h, w, c, dtype=torch.uint8, device=a.device)
    _call("mnk_nhwc_to_u8", a, _p(a), ld, _p(out), n * h * w, c)
    return out


def conv1x1_sigmoid_u8(x, weight, bias, cin, b):
    """Conv1x1SigmoidFn's forward (act = 1) written as uint8 (B, d, H, W, Cout): the same kernel with a byte epilogue.
    No autograd node: the caller is in evaluation mode under no_grad."""
    _check_device(x)
    n, h, w, ld = x.shape
    cout = weight.shape[0]
    out = torch.empty(b, n // b, h, w, cout, dtype=torch.uint8, device=x.device)
    _call("mnk_conv1x1_fwd_u8", x, _p(x), ld, cin, _p(weight), _p(bias), _p(out), b, n // b, h, w, cout)
    return out


class ToActPairFn(_Fn):
    """ToActFn of StackedBatch(a, b): one act, its two halves written by one conversion launch each."""

    @staticmethod
    def forward(ctx, a5, b5, step):
        _check_device(a5)
        a5, b5 = a5.contiguous().float(), b5.contiguous().float()
        b, c, d, h, w = a5.shape
        out = torch.empty(2 * b * d, h // step, w // step, ceil4(c), dtype=torch.float32, device=a5.device)
        for i, src in enumerate((a5, b5)):
            _call("mnk_ncdhw_to_nhwc", src, _p(src), _p(out[i * b * d:]), b, c, d, h, w, step, ceil4(c))
        ctx.meta = (b, c, d, h, w, step)
        return out

    @staticmethod
    def backward(ctx, g):
        b, c, d, h, w, step = ctx.meta
        if step != 1:
            raise NotImplementedError("gradient w.r.t. a down-scaled input image is never consumed by the reference")
        g = g.contiguous()
        outs = [None, None]
        for i in range(2):
            if ctx.needs_input_grad[i]:
                outs[i] = torch.empty(b, c, d, h, w, dtype=torch.float32, device=g.device)
                _call("mnk_nhwc_to_ncdhw", g, _p(g[i * b * d:]), g.shape[-1], _p(outs[i]), b, c, d, h, w)
        return outs[0], outs[1], None


class FromActFn(_Fn):
    """act -> (B,C,D,H,W)."""

    @staticmethod
    def forward(ctx, a, c, b):
        n, h, w, ld = a.shape
        d = n // b
        out = torch.empty(b, c, d, h, w, dtype=torch.float32, device=a.device)
        _call("mnk_nhwc_to_ncdhw", a, _p(a), ld, _p(out), b, c, d, h, w)
        ctx.meta = (b, c, d, h, w, ld)
        return out

    @staticmethod
    def backward(ctx, g):
        b, c, d, h, w, ld = ctx.meta
        g = g.contiguous()
        out = torch.empty(b * d, h, w, ld, dtype=torch.float32, device=g.device)
        _call("mnk_ncdhw_to_nhwc", g, _p(g), _p(out), b, c, d, h, w, 1, ld)
        return out, None, None


class Concat2PairFn(_Fn):
    """Concat2Fn for the batched discriminator pass [generated | real] (mnk.engine.fused_pair_losses): `a` holds 2B frames, `b`
    (the key-point embedding, the same for both halves) B frames: out[n] = [a[n] | b[n mod B]].  The reference's two calls
    embed the same key points twice (train.py:43-45); here the embedding is made once, and its gradient is the sum of the two
    halves -- no concatenated key-point tensors, none of their backward additions."""

    @staticmethod
    def forward(ctx, a, ca, b, cb):
        n, h, w, _ = a.shape
        assert b.shape[0] * 2 == n and b.shape[1:3] == a.shape[1:3]
        out = torch.empty(n, h, w, ceil4(ca + cb), dtype=torch.float32, device=a.device)
        _call("mnk_concat2_fwd", a, _p(a), a.shape[-1], ca, _p(b), b.shape[-1], cb, n // 2, _p(out), out.shape[-1], n, h * w)
        ctx.meta = (ca, cb, a.shape[-1], b.shape[-1])
        return out

    @staticmethod
    def backward(ctx, g):
        ca, cb, lda, ldb = ctx.meta
        g = g.contiguous()
        n, h, w, ld = g.shape
        ga = torch.empty(n, h, w, lda, dtype=torch.float32, device=g.device)
        gb = torch.empty(n // 2, h, w, ldb, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[2] else None
        _call("mnk_concat2_bwd", g, _p(g), ld, ca, cb, n // 2, _p(ga), lda, _p(gb), ldb, n, h * w)
        return ga, None, gb, None


class Concat2Fn(_Fn):
    """torch.cat([a, b], dim=channel) on acts (modules/util.py:185 for the last decoder stage)."""

    @staticmethod
    def forward(ctx, a, ca, b, cb):
        n, h, w, _ = a.shape
        out = torch.empty(n, h, w, ceil4(ca + cb), dtype=torch.float32, device=a.device)       # one launch, pads included
        _call("mnk_concat2_fwd", a, _p(a), a.shape[-1], ca, _p(b), b.shape[-1], cb, n, _p(out), out.shape[-1], n, h * w)
        ctx.meta = (ca, cb, a.shape[-1], b.shape[-1])
        return out

    @staticmethod
    def backward(ctx, g):
        ca, cb, lda, ldb = ctx.meta
        g = g.contiguous()
        n, h, w, ld = g.shape
        ga = torch.empty(n, h, w, lda, dtype=torch.float32, device=g.device)
        gb = torch.empty(n, h, w, ldb, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[2] else None
        _call("mnk_concat2_bwd", g, _p(g), ld, ca, cb, n, _p(ga), lda, _p(gb), ldb, n, h * w)
        return ga, None, gb, None


# ----------------------------------------------------------------------------------------------------------------
# 3x3 convolution
# ----------------------------------------------------------------------------------------------------------------
_PACK_CACHE = {}
_PACK_EPOCH = [0]
_PACK_REG = {}                     # id(parameter) -> _PackEntry
_PACK_TABLE = {"dirty": True, "descs": None, "n": 0, "tiles": 0, "entries": (), "kxk": (), "keep": []}
_PACK_REG_VERSION = [0]            # bumped whenever an entry (or one of its buffers) is created or dropped


def invalidate_packed_weights():
    """Parameters were written behind the library's back (`p.data.copy_`, a custom update): drop every packed copy --
    the inference-side cache (keyed by this epoch) and the freshness of the training-side registry.  Optimiser steps do
    this by themselves (hook below), for the parameters of that optimiser."""
    _PACK_EPOCH[0] += 1
    for e in _PACK_REG.values():
        e.stamp = None


def bump_inference_epoch():
    """the no-grad cache only (a replayed training iteration re-packs its own weights on the device)"""
    _PACK_EPOCH[0] += 1


def _after_optimizer_step(opt, args, kwargs):
    """Global post-step hook of torch.optim: the stepped optimiser's parameters changed (fused optimisers do not bump
    `Tensor._version`, so the version check alone cannot see it).  An optimiser that wrote the packed layouts itself
    (mnk.optim.MnkAdam) hands its entries over to be stamped fresh."""
    _PACK_EPOCH[0] += 1
    # hand-overs of a backward pass that nobody picked up (a gradient that autograd summed with another one first) hold GPU
    # tensors: a user-owned loop -- the reference's train.py on these modules -- never calls clear_dz_stats()
    _DZ_STATS.clear()
    for g in opt.param_groups:
        for p in g["params"]:
            e = _PACK_REG.get(id(p))
            if e is not None:
                e.stamp = None
    fresh = getattr(opt, "_mnk_fresh_entries", None)
    if fresh:
        for e in fresh:
            w = e.wref()
            e.partial = adam_desc_flags(e) & 8 != 0      # what the kernel's table said (it is keyed by the registry version)
            if w is not None and e.wptr == w.data_ptr():
                e.stamp = w._version
        opt._mnk_fresh_entries = ()


try:  # any torch optimiser step anywhere invalidates what it touched
    from torch.optim.optimizer import register_optimizer_step_post_hook as _reg_hook
    _reg_hook(_after_optimizer_step)
except Exception:  # pragma: no cover - older torch: TrainStep still invalidates explicitly
    pass


# ---- gradient sinks: parameters whose gradient a kernel writes straight into an optimiser-owned flat buffer ------------
_SINKS = {}                        # id(parameter) -> weakref to the owning mnk.optim.MnkAdam


def register_grad_sink(p, owner):
    _SINKS[id(p)] = weakref.ref(owner)


def unregister_grad_sinks(ids, owner_id):
    for i in ids:
        r = _SINKS.get(i)
        if r is not None and (r() is None or id(r()) == owner_id):
            _SINKS.pop(i, None)


def sink_owner(p):
    r = _SINKS.get(id(p))
    return r() if r is not None else None


def wgrad_sink_owner(p):
    """the owner whose sink takes p's weight gradient in THIS backward pass, or None (autograd gets dW): an MnkAdam always, a
    mnk.optim.GradSinks only while the drop-in runner's phase B / C runs (FlatGrads.defers_wgrad)"""
    o = sink_owner(p)
    return o if o is not None and o.defers_wgrad else None


def pack_registry_version():
    return _PACK_REG_VERSION[0]


def pack_entry_of(p):
    """the training-side packed-weight entry of a 3x3 convolution weight, if a training forward has created one"""
    e = _PACK_REG.get(id(p))
    if e is not None and e.wref() is p and e.wptr == p.data_ptr():
        return e
    return None


def adam_desc_flags(e):
    """MnkAdamDesc::flags of a packed-weight entry, without the gt bits: bit 0 = the packs of the sub-pixel forms, bit 3
    (MNK_ADAM_UP1X1) = leave the dead slices of a 1 x 1 source alone.  One place for mnk.optim.MnkAdam and AdoptedAdam."""
    up = bool(e.meta[3])
    return int(up) | (8 if up and e.dead1x1 else 0)


def subpixel(ups):
    """UpBlock3D convolutions run in their sub-pixel forms (mnk_conv3x3_up_*) -- 13.87 -> 12.62 ms per step in round 2; the 3x3
    convolution over the up-sampled view stays for the operands the sub-pixel kernels do not take (a residual input) and, for
    A/B runs, behind the library's "up_subpixel" tuning value (MNK_TUNING=up_subpixel=0 or mnk_set_tuning), whose LIVE value
    this function reads (mnk_get_tuning: the library's weight-gradient plans follow the same integer)."""
    if not ups:
        return False
    # read once per library handle and per mnk_set_tuning call made through it (a ctypes round trip per up-sampled
    # convolution of every eager forward, and a value that could change between a forward and its backward)
    lib = _lib.lib()
    epoch = getattr(lib, "tuning_epoch", 0)
    hit = getattr(lib, "_subpixel_cache", None)
    if hit is None or hit[0] != epoch:
        import ctypes
        v = ctypes.c_int(1)
        lib.call("mnk_get_tuning", b"up_subpixel", ctypes.byref(v))
        hit = lib._subpixel_cache = (epoch, bool(v.value))
    return hit[1]


# mnk.dropin.EvalRunner and mnk.animation.AnimationSession capture an evaluation forward with FROZEN weights: the cached packed
# weights / evaluation-mode norm coefficients are used (and their addresses recorded) instead of re-made inside the graph; they
# re-capture when weights_fingerprint() changes.  Written by mnk.graphs.frozen_weights() only
FROZEN_CAPTURE = [False]


def weights_fingerprint(tensors):
    """what a frozen-weight program over `tensors` depends on: the pack and norm-coefficient epochs, and per tensor its version and
    its address (`p.data = ...`, module.float() / .to() swap the storage the graph reads and keep _version)"""
    return (_PACK_EPOCH[0], _BN_EVAL_EPOCH[0], tuple((t._version, t.data_ptr()) for t in tensors))


def held_eval_coeffs(modules):
    """the cached evaluation-mode norm coefficients of the modules' layers.  A frozen graph reads them by address and the cache
    keeps ONE entry per layer (a call on another stream replaces it): a frozen program holds what it reads"""
    return [_BN_EVAL.get(id(b)) for m in modules for b in m.buffers()]


# The entry points of one form of the forward / data-gradient implicit GEMM (csrc/conv3x3.hip): packed size and pack of its
# weights, the three size queries (splits: None where the form has none), the launch, the launch that also leaves the backward
# statistics of the BatchNorm in front (None: no such form), and the phases of a launch.
_GemmForm = namedtuple("_GemmForm", "packed pack ws stats splits launch bn_launch phases", defaults=(None, 1))


# the only place these names are chosen: everything below asks for a form
_FORMS = {
    # 3x3 / pad 1, forward and (on dy, with the data-gradient pack) data gradient
    "3x3": _GemmForm("mnk_conv3x3_packed_floats", "mnk_conv3x3_pack_fwd", "mnk_conv3x3_workspace_floats",
                     "mnk_conv3x3_stats_floats", "mnk_conv3x3_splits", "mnk_conv3x3_fwd", "mnk_conv3x3_dgrad_bnstats"),
    # [nearest x2 -> 3x3 / pad 1] in its sub-pixel forms; (H, W) of their calls = the LOW resolution
    "up": _GemmForm("mnk_conv3x3_up_packed_floats", "mnk_conv3x3_up_pack_fwd", "mnk_conv3x3_up_workspace_floats",
                    "mnk_conv3x3_up_stats_floats", "mnk_conv3x3_up_splits", "mnk_conv3x3_up_fwd", phases=4),
    "up_dgrad": _GemmForm("mnk_conv3x3_up_dgrad_packed_floats", "mnk_conv3x3_up_pack_dgrad",
                          "mnk_conv3x3_up_dgrad_workspace_floats", "mnk_conv3x3_up_dgrad_stats_floats", None,
                          "mnk_conv3x3_up_dgrad", "mnk_conv3x3_up_dgrad_bnstats"),
    # K x K, any pad, one source (the discriminator); its data gradient is the same form on dy
    "kxk": _GemmForm("mnk_conv2d_packed_floats", "mnk_conv2d_pack_fwd", "mnk_conv2d_workspace_floats", "mnk_conv2d_stats_floats",
                     None, "mnk_conv2d_fwd"),
}


def _cached_pack(kind, weight, shape, nfloats, make):
    """One cached pack of a conv weight for NO-GRAD forwards: `make(wp)` launches the pack into a fresh buffer of `nfloats`.
    kind: "fwd" or "up" (one entry per parameter: `up` is part of the stored shape, so either form replaces the other) or
    ("skinny", bf16) (an entry of its own per precision).  An entry is valid for one parameter version, storage and optimiser
    epoch and dies with its parameter.  Under hipGraph capture the cache is bypassed: the pack launch is recorded INTO the graph
    (its buffer lives in the graph's memory pool), so every replay re-packs from the live parameter -- a replay after
    load_state_dict / an in-place write can never combine old packed weights with new normalisation parameters.  (A capture with
    frozen weights, FROZEN_CAPTURE, takes the cached pack and records its address.)"""
    if weight.is_cuda and torch.cuda.is_current_stream_capturing() and not FROZEN_CAPTURE[0]:
        wp = torch.empty(nfloats, dtype=torch.float32, device=weight.device)
        make(wp)
        return wp
    key = (id(weight), weight.device, "fwd" if kind == "up" else kind)
    ver = (weight._version, _PACK_EPOCH[0], weight.data_ptr())
    shape = (kind, shape)
    hit = _PACK_CACHE.get(key)
    if hit is not None and hit[0] == ver and hit[1] == shape and hit[3]() is weight:
        return hit[2]
    wp = torch.empty(nfloats, dtype=torch.float32, device=weight.device)
    make(wp)
    if hit is None:
        weakref.finalize(weight, _PACK_CACHE.pop, key, None)      # no entry (and no packed buffer) outlives its parameter
    _PACK_CACHE[key] = (ver, shape, wp, weakref.ref(weight))
    return wp


def _packed_fwd_weight(weight, cout, c0, c1, up=False):
    """Packed [Cout][chunk][tap][16] copy of a conv weight for NO-GRAD forwards (inference loops), cached by _cached_pack.
    Training forwards never use this cache (they take the registry entry of _pack_entry: re-packed once per iteration by
    repack_registered(), or per call in a user-owned loop)."""
    form = _FORMS["up" if up else "3x3"]
    return _cached_pack("up" if up else "fwd", weight, (cout, c0, c1), _query(form.packed, cout, c0, c1),
                        lambda wp: _call(form.pack, weight, _p(weight), _p(wp), cout, c0, c1))


def up1x1_dead_taps(n, hs, ws):
    """An up-sampled convolution of n frames on an hs x ws LOW-resolution source leaves the dead pseudo taps of a 1 x 1 source out
    (the library's rule, mnk_up1x1_dead_taps: its weight-gradient GEMM writes no partials for them, so their readers must not
    load them).  Read once per library handle and mnk_set_tuning call, like subpixel()."""
    if hs != 1 or ws != 1:
        return False
    lib = _lib.lib()
    epoch = getattr(lib, "tuning_epoch", 0)
    hit = getattr(lib, "_up1x1_cache", None)
    if hit is None or hit[0] != epoch:
        hit = lib._up1x1_cache = (epoch, {})
    if n not in hit[1]:
        hit[1][n] = bool(lib.query("mnk_up1x1_dead_taps", n, 1, 1))
    return hit[1][n]


class _PackEntry:
    """Persistent packed copies (forward + data-gradient layouts) of one conv parameter used by training forwards.
    The three fields of an up-sampled convolution that runs on a 1 x 1 source (up1x1_dead_taps):
      dead1x1  the geometry the weight was LAST used at lets the optimiser kernel leave the dead slices of the packs alone
               (MnkAdamDesc bit 3); a change bumps pack_registry_version(), which the optimisers' tables are keyed by;
      partial  the last emission did: the dead slices hold finite values of an earlier, full pack -- only meaningful while the
               entry is fresh (a stale entry is packed in full before any use);
      full     a forward has needed the dead slices of a partial entry (the same weight on a larger source): it was packed in
               full, and dead1x1 stays off for this weight from then on."""
    __slots__ = ("wref", "wptr", "meta", "ntaps", "wp", "wd", "stamp", "dead1x1", "partial", "full", "__weakref__")

    def same(self, weight, meta, ntaps):
        return self.wref() is weight and self.wptr == weight.data_ptr() and self.meta == meta and self.ntaps == ntaps

    def fresh(self, weight, meta, need, ntaps=9):
        return (self.same(weight, meta, ntaps) and self.stamp is not None and self.stamp == weight._version
                and all(self.wd[i] is not None for i in (0, 1) if need[i]))

    def pack(self):
        """one launch for this layer alone (mnk_conv2d_pack_all: a K x K weight, ntaps = K * K <= 16)"""
        w, (cout, c0, c1, _) = self.wref(), self.meta
        _call("mnk_conv2d_pack_all", w, _p(w), _p(self.wp), _p(self.wd[0]), _p(self.wd[1]), cout, c0, c1, self.ntaps)



def _note_geometry(e, dead):
    """A forward uses entry `e`; dead: on a geometry whose dead slices nobody reads (up1x1_dead_taps).  Records the geometry for
    the next optimiser step and answers whether the packs can be used as they are -- False: this use needs slices that the last
    emission left out."""
    want = bool(dead) and not e.full
    usable = want or not e.partial
    if not usable:
        e.full, want = True, False
    if e.dead1x1 != want:
        e.dead1x1 = want
        _PACK_REG_VERSION[0] += 1          # the optimisers' descriptor tables carry the bit
    return usable


def _pack_entry(weight, cout, c0, c1, need, up=False, ntaps=9, dead1x1=False):
    """The (packed, up to date) registry entry of `weight`: packs with one per-layer launch unless the entry is fresh
    (repack_registered() ran since the last optimiser step).  up: the packs of the sub-pixel forms of an up-sampled
    convolution (mnk_conv3x3_up_fwd / _up_dgrad) instead of the 3x3 layouts.  ntaps != 9: a K x K weight (ConvKxKFn).
    dead1x1: this forward and its backward run on a 1 x 1 source (up1x1_dead_taps; see _PackEntry)."""
    meta = (cout, c0, c1, bool(up))
    kxk = ntaps != 9
    form, dform = (_FORMS["up"], _FORMS["up_dgrad"]) if up else (_FORMS["3x3"], _FORMS["3x3"])
    e = _PACK_REG.get(id(weight))
    known = e is not None and e.same(weight, meta, ntaps)
    # (a fresh entry whose last emission was partial and whose dead slices are needed now takes the stale entry's way: one launch)
    usable = _note_geometry(e, dead1x1) if known else True
    if usable and e is not None and e.fresh(weight, meta, need, ntaps):
        return e
    if (known
            and all(e.wd[i] is not None for i in (0, 1) if need[i])):
        # a known layer gone stale (an optimiser stepped): the first such layer of an iteration re-packs EVERY registered
        # parameter in one launch -- a user-owned loop (the reference's train.py) then pays one pack launch per iteration
        # instead of one (to three) per convolution, as mnk.engine.TrainStep does at the start of its iterations
        if repack_registered() and e.fresh(weight, meta, need, ntaps):
            return e
    if e is None or not e.same(weight, meta, ntaps):
        e = _PackEntry()
        e.wref, e.wptr, e.meta, e.wd, e.stamp = weakref.ref(weight), weight.data_ptr(), meta, [None, None], None
        e.ntaps = ntaps
        e.dead1x1, e.partial, e.full = bool(dead1x1), False, False
        nf = _query(_FORMS["kxk"].packed, cout, c0, c1, ntaps) if kxk else _query(form.packed, cout, c0, c1)
        e.wp = torch.empty(nf, dtype=torch.float32, device=weight.device)
        key = id(weight)
        _PACK_REG[key] = e
        weakref.finalize(weight, _drop_pack_entry, key, weakref.ref(e))
        _PACK_TABLE["dirty"] = True
        _PACK_REG_VERSION[0] += 1
    for i, cc in enumerate((c0, c1)):
        if need[i] and e.wd[i] is None:
            if kxk:
                nd = _query(_FORMS["kxk"].packed, cc, cout, 0, ntaps)
            else:
                nd = _query(dform.packed, cout, cc) if up else _query(dform.packed, cc, cout, 0)
            e.wd[i] = torch.empty(nd, dtype=torch.float32, device=weight.device)
            _PACK_TABLE["dirty"] = True
            _PACK_REG_VERSION[0] += 1
    if kxk:
        e.pack()
    elif up:
        _call(form.pack, weight, _p(weight), _p(e.wp), cout, c0, c1)
        for i, (cs, cc) in enumerate(((0, c0), (c0, c1))):
            if e.wd[i] is not None:
                _call(dform.pack, weight, _p(weight), _p(e.wd[i]), cout, c0 + c1, cs, cc)
    else:
        _call("mnk_conv3x3_pack_all", weight, _p(weight), _p(e.wp), _p(e.wd[0]), _p(e.wd[1]), cout, c0, c1)
    e.stamp = None            # only repack_registered() vouches for freshness: a user-owned loop packs on every call
    e.partial = False         # (every pack launch of this module writes all slices; only the optimiser kernel leaves some out)
    return e


def _drop_pack_entry(key, eref):
    if _PACK_REG.get(key) is eref():
        _PACK_REG.pop(key, None)
        _PACK_TABLE["dirty"] = True
        _PACK_REG_VERSION[0] += 1


def repack_registered(only_if_stale=False):
    """Re-pack EVERY registered conv parameter: the 3x3 ones in one launch (mnk_conv3x3_pack_multi), each K x K one (the
    discriminator's four) with a launch of its own -- the start of a training
    iteration (mnk.engine.TrainStep): ~40 per-layer pack launches become one.  Parameters first seen later in the
    iteration (and everything, when called under stream capture before the table exists) fall back to per-layer packs.
    only_if_stale: nothing to do when every entry is still fresh (the optimiser kernel of mnk.optim wrote the packs)."""
    t = _PACK_TABLE
    if only_if_stale and _PACK_REG:
        stale = False
        for e in _PACK_REG.values():
            w = e.wref()
            if w is not None and (e.stamp is None or e.stamp != w._version or e.wptr != w.data_ptr()):
                stale = True
                break
        if not stale:
            return False
    if t["dirty"]:
        entries = [e for e in _PACK_REG.values() if e.wref() is not None and e.wptr == e.wref().data_ptr()]
        if not entries:
            return False
        dev = entries[0].wp.device
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return False                     # building the table needs a host-to-device copy
        entries = [e for e in entries if e.wp.device == dev]
        kxk = tuple(e for e in entries if e.ntaps != 9)
        entries = [e for e in entries if e.ntaps == 9]
        rec = np.zeros(len(entries), dtype=np.dtype([("p", "<u8", 4), ("i", "<i4", 6)]))
        tiles = 0
        for k, e in enumerate(entries):
            cout, c0, c1, up = e.meta
            rec["p"][k] = (e.wptr, e.wp.data_ptr(), e.wd[0].data_ptr() if e.wd[0] is not None else 0,
                           e.wd[1].data_ptr() if e.wd[1] is not None else 0)
            rec["i"][k] = (cout, c0, c1, tiles, int(up), 0)
            tiles += ((ceil16(c0) + (ceil16(c1) if c1 else 0)) // 16) * ((cout + 15) // 16)
        descs = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
        t["keep"].append(descs)              # captured graphs hold raw pointers to earlier tables: never free them
        t.update(dirty=False, descs=descs, n=len(entries), tiles=tiles, entries=tuple(entries), kxk=kxk)
    if not t["n"] and not t["kxk"]:
        return False
    if t["n"]:
        _call("mnk_conv3x3_pack_multi", t["descs"], _p(t["descs"]), t["n"], t["tiles"])
    for e in t["kxk"]:
        if e.wref() is not None:
            e.pack()
    for e in t["entries"] + t["kxk"]:
        w = e.wref()
        e.partial = False
        if w is not None:
            e.stamp = w._version
    return True


# a split-K convolution whose partials a small-layer BatchNorm will sum: y.data_ptr() -> _SplitPending
_SPLIT_PENDING = {}


# the partials of a deferred split-K launch: [splits][phases][M][ld] floats at `ws`, the bias not added
_SplitPending = namedtuple("_SplitPending", "ws splits phases bias")
_NO_SPLIT = _SplitPending(None, 0, 1, None)      # what a BatchNorm with nothing pending tells its kernel


def _drop_stale_split_pending():
    """Before a launch that may use the scratch workspace: the BatchNorm of an earlier deferred split-K convolution never ran -- an
    exception between the two launches (the entry is popped by that BatchNorm; nothing else may run in between).  The partial sums
    are gone with the scratch buffer; drop the entry -- a retry of the forward pass must not be poisoned by the failed one -- and
    say so."""
    if _SPLIT_PENDING:
        import warnings
        warnings.warn("dropping the deferred split-K partial sums of %d convolution(s) whose BatchNorm never ran (an "
                      "exception between a convolution and its normalisation layer?)" % len(_SPLIT_PENDING))
        _SPLIT_PENDING.clear()


def _small_sync(rows):
    """several ranks with the peer-to-peer exchange up: a small layer's backward is mnk_bn_small_bwd_sync (one launch)"""
    return mdist.active() and 1 < rows <= _query("mnk_bn_small_rows") and _sync_handle() is not None


def small_bn(rows, training=True, c=0):
    """the one-launch BatchNorm forms of small layers apply: training statistics, few pixel rows (per rank), and either a
    single rank or -- several ranks -- the peer-to-peer exchange up (mnk_bn_small_fwd_sync / _bwd_sync carry it inside the
    launch; a layer of c channels must fit a mailbox row)"""
    if not (training and 1 < rows <= _query("mnk_bn_small_rows")):
        return False
    return not mdist.active() or _sync_handle(c) is not None


def _gemm_launch(form, x0, c0, x1, c1, wp, bias, residual, n, h, w, cout, flags=0, stats=False, defer=False, bn=None, kxk=None):
    """One forward / data-gradient GEMM launch of `form` (_FORMS): sizes its workspace (and, with `stats`, its statistics buffer)
    by the form's queries, takes the scratch workspace and launches.  -> (y, statistics partials or None).
    (n, h, w): the map of the form's calls -- the LOW resolution for "up" (y is twice as large) and "up_dgrad"; a data gradient
    reads dy as x0 (c0 = its channels) and writes cout = the source's channels.
    defer: a launch that splits along K leaves its partials in the workspace for the BatchNorm that follows (_SPLIT_PENDING).
    bn: the _BnRecord of the BatchNorm in front of a data gradient, whose backward statistics the launch leaves where its plan
    has a statistics form (else an ordinary launch).  kxk: (hi, wi, kh, kw, pad) of the "kxk" form."""
    f = _FORMS[form]
    _drop_stale_split_pending()
    up = form == "up"
    y = torch.empty(n, h * 2 if up else h, w * 2 if up else w, ceil4(cout), dtype=torch.float32, device=x0.device)
    size = (n, h, w, c0, cout) if form == "up_dgrad" else (n, h, w, c0, c1, cout, kxk[2] * kxk[3]) if kxk else (n, h, w, c0, c1, cout)
    nws = _query(f.ws, *size)
    ws = SCRATCH.get("ws", nws, x0) if nws else None
    nst = _query(f.stats, *size) if stats or bn is not None else 0
    st = torch.empty(nst, dtype=torch.float32, device=x0.device) if nst else None      # lives until the norm layer reads it
    deferred = defer and nws
    if deferred:
        flags |= 4                       # MNK_CONV_DEFER_SPLITK
    # (plain positional calls: this is the host-bound evaluation loops' path)
    ld1, ldr = x1.shape[-1] if x1 is not None else 0, residual.shape[-1] if residual is not None else 0
    # MNK_CONV_BF16_TRAIN on an entry that has no `flags` argument: its _ex form (the plain names are the _ex forms with 0)
    ex = ("_ex", (flags & 16,)) if flags & 16 else ("", ())
    if bn is not None and st is not None:
        tail = (_p(ws), nws, _p(st), _p(bn.y), bn.y.shape[-1], _p(bn.mean), _p(bn.invstd), _p(bn.scale), _p(bn.beta), float(bn.slope))
        if form == "3x3":
            _call(f.bn_launch + ex[0], x0, _p(x0), x0.shape[-1], c0, _p(wp), _p(residual), ldr, _p(y), y.shape[-1], n, h, w, cout,
                  *tail, *ex[1])
        else:
            _call(f.bn_launch + ex[0], x0, _p(x0), x0.shape[-1], c0, _p(wp), _p(y), y.shape[-1], n, h, w, cout, *tail, *ex[1])
    elif form == "3x3":
        _call(f.launch, x0, _p(x0), x0.shape[-1], c0, _p(x1), ld1, c1, flags, _p(wp), _p(bias), _p(residual), ldr, _p(y), y.shape[-1],
              n, h, w, cout, _p(ws), nws, _p(st))
    elif up:
        _call(f.launch, x0, _p(x0), x0.shape[-1], c0, _p(x1), ld1, c1, flags, _p(wp), _p(bias), _p(y), y.shape[-1], n, h, w, cout,
              _p(ws), nws, _p(st))
    elif form == "up_dgrad":
        _call(f.launch + ex[0], x0, _p(x0), x0.shape[-1], c0, _p(wp), _p(y), y.shape[-1], n, h, w, cout, _p(ws), nws, *ex[1])
    else:
        _call(f.launch, x0, _p(x0), x0.shape[-1], c0, _p(x1), ld1, c1, flags, *kxk, _p(wp), _p(bias), _p(residual), ldr, _p(y),
              y.shape[-1], n, h, w, cout, _p(ws), nws, _p(st))
    if deferred:
        _SPLIT_PENDING[y.data_ptr()] = _SplitPending(ws, _query(f.splits, *size), f.phases, bias)
    return y, st


# ---- opt-in bf16 inference ------------------------------------------------------------------------------------------------------
# the precision of the 3x3 / sub-pixel forward GEMMs launched under torch.no_grad(): "fp32", or "bf16" = MNK_CONV_BF16 (operands
# rounded to nearest-even bf16 in the loaders, exact products, fp32 accumulation; include/monkeynet_hip.h).  Everything else --
# 1x1, grouped 1x1, embedding, warp, soft-argmax, norm layers -- is memory-bound and stays fp32.
PRECISIONS = ("fp32", "bf16")


def bf16_excluded(cin, cout):
    """layers that keep the fp32 form inside inference_precision("bf16"): the 16-wide tile of conv3x3_igemm16_kernel (Cout <= 16) fed
    by 64 or more input channels -- the dense-motion mask head, 76 or 98 -> 13.  Measured (profiles/bf16_inference.txt, section 3a)
    the one-pass form gains 1.02 ... 1.17 x there and missed the per-layer gate on bair batch 512 (2M rows: 0.735 -> 0.718 ms,
    spread 0.021).  The narrower key-point heat-map head (35 -> 10; 1.16 ... 1.24 x, outside the gate's range) keeps the flag."""
    return cout <= 16 and cin >= 64

def check_precision(precision):
    if precision not in PRECISIONS:
        raise ValueError("precision must be one of %s, not %r" % (PRECISIONS, precision))
    return precision


# ---- the evaluation options: precision, norm fusion, skinny convolutions ------------------------------------------------------------
# what a forward launched under torch.no_grad() runs with.  One value per process, not per thread: a scope opened in one thread also
# changes the convolutions another thread launches meanwhile.  The loops here are single-threaded; keep a default forward of another
# thread out of a scope.
EvalOptions = namedtuple("EvalOptions", "precision fuse_norm skinny", defaults=("fp32", False, False))


class _EvalState:
    __slots__ = EvalOptions._fields


_EVAL = _EvalState()
_EVAL.precision, _EVAL.fuse_norm, _EVAL.skinny = EvalOptions()


def current_eval_options():
    return EvalOptions(_EVAL.precision, _EVAL.fuse_norm, _EVAL.skinny)


class eval_options:
    """Context manager: `with eval_options(precision="bf16", skinny=True):` sets the given fields (None: the field stays as it is)
    for the forwards launched inside; `with eval_options(*opts):` sets all three from an EvalOptions.  The previous values of the
    fields it set are restored on exit, also after an exception.  inference_precision, eval_norm_fusion and eval_skinny_conv
    (below) are this scope with one field and say what each field does."""

    def __init__(self, precision=None, fuse_norm=None, skinny=None):
        self.precision = None if precision is None else check_precision(precision)
        self.fuse_norm = None if fuse_norm is None else bool(fuse_norm)
        self.skinny = None if skinny is None else bool(skinny)

    def __enter__(self):
        self.previous = [(f, getattr(_EVAL, f)) for f in EvalOptions._fields if getattr(self, f) is not None]
        for f, _ in self.previous:
            setattr(_EVAL, f, getattr(self, f))
        return self

    def __exit__(self, *exc):
        for f, v in self.previous:
            setattr(_EVAL, f, v)
        return False


def inference_precision(precision):
    """Context manager: inside `with inference_precision("bf16"):` every 3x3 and sub-pixel forward convolution launched under
    torch.no_grad() runs its products in one bf16 pass.  A convolution called with gradients enabled inside the scope raises
    RuntimeError: the backward kernels are fp32 and would not differentiate what was computed.  Outside any scope the precision
    is fp32."""
    return eval_options(precision=check_precision(precision))


def current_precision():
    return _EVAL.precision


# ---- opt-in bf16 (mixed-precision) training ---------------------------------------------------------------------------------------
# the precision of the three GEMMs of a 3x3 / sub-pixel convolution NODE -- forward (MNK_CONV_BF16_TRAIN, training statistics
# included), data gradient (the same flag) and weight gradient (MNK_WGRAD_BF16) -- that is called with gradients enabled.  The
# operands are rounded to nearest-even bf16 in the loaders, products are exact, accumulation is fp32; weights, gradients, activations
# and optimiser state stay fp32 in memory, and so does every other layer: the discriminator's 4x4 convolutions and first-block
# kernels, 1x1 and grouped 1x1 convolutions, norm layers, warp, embedding, soft-argmax, losses, Adam.
_TRAIN_PRECISION = ["fp32"]


class training_precision:
    """Context manager: inside `with training_precision("bf16"):` every 3x3 and sub-pixel convolution called with gradients
    enabled runs its forward products in one bf16 pass and records that on its autograd node; the node's data- and weight-gradient
    GEMMs follow the RECORDED value, also when backward() runs after the scope was left.  A node is bf16 in all three GEMMs or in
    none: bf16_excluded(cin, cout) decides at forward time.  Calls under torch.no_grad() are not touched (fp32 unless an
    inference_precision scope says otherwise), and inference_precision keeps its own semantics inside this scope.  Outside any
    scope the precision is fp32; the previous value is restored on exit, also after an exception.  One value per process, like
    inference_precision."""

    def __init__(self, precision):
        self.precision = check_precision(precision)

    def __enter__(self):
        self.previous = _TRAIN_PRECISION[0]
        _TRAIN_PRECISION[0] = self.precision
        return self

    def __exit__(self, *exc):
        _TRAIN_PRECISION[0] = self.previous
        return False


def current_training_precision():
    return _TRAIN_PRECISION[0]


def _fwd_launch_geometry(ups, up, h, w, c0, c1, cout):
    """-> (hq, wq, flags) of a forward launch on an (h, w) output.  up: the sub-pixel form, whose calls take the LOW resolution and
    no flags of the view; else bit 0 = nearest x2 up-sampled view, bit 1 = MNK_CONV_CLEAN_PADS -- every act this module produces
    has zero pad channels (tests/test_modules.py::test_pad_channels_are_written pins that), so the fast 3x3 loader applies.
    Bit 3 = MNK_CONV_BF16 inside inference_precision("bf16") (conv3x3 vouches for no_grad and an evaluation-mode norm layer), not
    for bf16_excluded layers: they stay fp32."""
    hq, wq, flags = (h // 2, w // 2, 0) if up else (h, w, int(bool(ups)) | 2)
    if _EVAL.precision == "bf16" and not bf16_excluded(c0 + c1, cout):
        flags |= 8
    return hq, wq, flags


def _conv_launch(x0, c0, x1, c1, ups, wp, bias, residual, n, h, w, cout, want_stats=False, up=False, eval_defer=False,
                 train_bf16=False):
    """One conv launch.  With want_stats the BatchNorm sums of the output come out of the conv epilogue (finished by a
    tiny second-stage kernel) instead of a separate pass over y; returns (y, sums or None).  up: `wp` holds the
    sub-pixel packs of an up-sampled convolution and (h, w) is the up-sampled size.  eval_defer: conv3x3(eval_bn=True)."""
    # a small layer whose BatchNorm follows at once (want_stats): that one-launch kernel makes its own statistics and,
    # when this convolution is split along K, also sums the partials -- no separate reduction, no epilogue statistics
    # (even sizes only: a pooling BatchNorm on an odd map -- 96 x 96 frames reach 3 x 3 -- takes the general kernels, and this
    # function does not know whether the BatchNorm that follows pools)
    small = want_stats and residual is None and small_bn(n * h * w, True, cout) and h % 2 == 0 and w % 2 == 0
    # evaluation mode: the norm layer that follows sums a split launch's partials itself
    evald = eval_defer and not want_stats and residual is None and h % 2 == 0 and w % 2 == 0
    assert not up or (ups and residual is None)
    hq, wq, flags = _fwd_launch_geometry(ups, up, h, w, c0, c1, cout)
    if train_bf16:
        flags = flags & ~8 | 16              # MNK_CONV_BF16_TRAIN: the node's decision (Conv3x3Fn.forward), statistics allowed
    y, st = _gemm_launch("up" if up else "3x3", x0, c0, x1, c1, wp, bias, residual, n, hq, wq, cout, flags, want_stats and not small,
                         small or evald)
    if small:
        return y, y.new_empty(0)
    sums = None
    if want_stats:
        nst = st.numel() if st is not None else 0
        if nst and not mdist.active():
            sums = st                          # per-block partials: finished together with the finalisation (bn_act)
        elif nst:
            sums = torch.empty(2 * cout, dtype=torch.float32, device=x0.device)
            sh = _sync_handle(cout)
            if sh is not None:                 # second stage + exchange over the ranks in one launch
                _call("mnk_bn_stats_finish_sync", x0, sh, _p(st), nst // (2 * y.shape[-1]), y.shape[-1], cout, None, _p(sums),
                      mdist.P2P_TIMEOUT_MS)
                _mark_reduced(sums)
            else:
                _call("mnk_bn_stats_finish", x0, _p(st), nst // (2 * y.shape[-1]), y.shape[-1], cout, _p(sums))
        elif mdist.active():
            sums = channel_sums(y, cout, sync=True)       # split-K layers: statistics by a pass over y
        else:
            sums = y.new_empty(0)              # split-K layers, single process: bn_act makes its own pass over y
    return y, sums


# statistics vectors that already hold the sums over the ranks (see _sync_handle): data pointer -> weak reference to the
# tensor.  The entry dies WITH the tensor (its finaliser removes it), so an unconsumed entry -- an exception mid-forward, a
# norm layer whose .training differs from the block's -- can never mark whatever the allocator puts at that address next
# (ADVICE r4).
_REDUCED = {}


def _mark_reduced(t):
    key = t.data_ptr()
    _REDUCED[key] = weakref.ref(t, lambda _r, key=key: _REDUCED.pop(key, None))


def _take_reduced(t):
    return _REDUCED.pop(t.data_ptr(), None) is not None


def _sync_handle(c=0):
    """The connected peer-to-peer exchange (csrc/p2p.hip) when the BatchNorm statistics of this process are exchanged by it: the
    statistics' second stage then carries the exchange itself (mnk_bn_*_sync: one launch instead of second stage + collective).
    c: the layer's channel count -- 2c sums must fit a mailbox row (mnk_p2p_max_floats: 1056 channels), wider layers take the
    collective path."""
    if not mdist.active():
        return None
    h = mdist.p2p_comm()
    if h is None or 2 * c > mdist._P2P["max"]:
        return None
    import ctypes
    return ctypes.c_void_p(h)


def channel_sums(a, c, sync=False):
    """[sum over pixels of a[..., :c], sum of squares] -> tensor (2c,).  sync: over the ranks, when the peer-to-peer exchange is
    up (the result is then registered in _REDUCED: no all-reduce behind it)."""
    rows = a.numel() // a.shape[-1]
    ld = a.shape[-1]
    nws = _query("mnk_bn_workspace_floats", rows, ld)
    ws = SCRATCH.get("ws", nws, a)
    sums = torch.empty(2 * c, dtype=torch.float32, device=a.device)
    h = _sync_handle(c) if sync else None
    if h is not None:
        _call("mnk_bn_stats_sync", a, h, _p(a), ld, rows, c, None, _p(sums), _p(ws), nws, mdist.P2P_TIMEOUT_MS)
        _mark_reduced(sums)
        return sums
    _call("mnk_bn_stats", a, _p(a), ld, rows, c, _p(sums), _p(ws), nws)
    return sums


# (dy tensor, its column sums) handed from BNActFn.backward to the Conv3x3Fn.backward that receives this very tensor
_DY_SUMS = [None]

# ---- backward statistics of a norm layer from the data-gradient GEMM behind it (round 4) ---------------------------------------
# bn_act() remembers, per OUTPUT tensor z of a training-mode BatchNorm that does not pool, what its backward statistics need
# (y, mean, inv-std, scale, beta, activation).  A convolution that consumes z keeps that record; its data-gradient launch --
# whose output IS dz when z has no other consumer -- then also leaves the column sums of g and g * xhat (mnk_conv3x3_dgrad_bnstats:
# the dz tile is in the GEMM's registers, only y is read), and hands them to the norm layer's backward under the dx tensor it
# returns.  The norm layer's backward looks its incoming gradient up: the very tensor -> one second-stage launch instead of a
# pass over y and dz + second stage; anything else (a second consumer made autograd add two gradients) -> the ordinary pass.
import weakref  # noqa: E402

_BN_OF = {}                               # id(z) -> (weak reference to z, _BnRecord); z = the tensor object callers hold
#                                           (a WeakKeyDictionary would compare tensors with ==)


def _bn_of(t):
    e = _BN_OF.get(id(t)) if t is not None else None
    return e[1] if e is not None and e[0]() is t else None


def _bind_bn(z, rec):
    key = id(z)
    _BN_OF[key] = (weakref.ref(z, lambda _r, key=key: _BN_OF.pop(key, None)), rec)
_LAST_BN = [None]                         # BNActFn.forward -> bn_act(): the record of the launch that just ran
_DZ_STATS = {}                            # dx.data_ptr() -> (dx, partials, rows, y.data_ptr(), dx._version); dx is held: a unique key
DZ_STATS_COUNT = [0, 0]                   # norm-layer backward passes that took the hand-over / that made their own pass (tests)


class _BnRecord:
    __slots__ = ("y", "mean", "invstd", "scale", "beta", "c", "slope")

    def __init__(self, y, mean, invstd, scale, beta, c, slope):
        self.y, self.mean, self.invstd, self.scale, self.beta, self.c, self.slope = y, mean, invstd, scale, beta, c, slope


def clear_dz_stats():
    """drop hand-overs that no norm layer picked up (their gradient was summed with another one first): start of an iteration"""
    _DZ_STATS.clear()
    _REDUCED.clear()


def handover_state():
    """The ONE-SHOT hand-overs between two adjacent calls of this module (producer -> the very next consumer), by name, with what
    is left in them.  Between two forward / backward passes every one of them is empty: anything left over is a producer whose
    consumer never ran (an exception in between, a caller that broke the `conv3x3(..., eval_bn=True)` -> `bn_act` contract) and
    would be picked up by an unrelated later call.  tests/test_step.py and tests/test_inference.py assert {} after whole passes.
    (Not listed: caches and registries keyed by tensor identity + version -- _PACK_*, _BN_EVAL, _BN_OF, _SINKS, _REDUCED,
    _DZ_STATS: entries die with their tensors or at clear_dz_stats().)"""
    slots = {
        "_SPLIT_PENDING (split-K convolution -> the norm layer that sums its partials)": len(_SPLIT_PENDING),
        "_FUSED_PENDING (convolution that applied its norm layer -> the bn_act that hands z through)": len(_FUSED_PENDING),
        "_LAST_BN (BNActFn.forward -> bn_act)": _LAST_BN[0],
        "_DY_SUMS (BNActFn.backward -> Conv3x3Fn.backward)": _DY_SUMS[0],
        "_SKIP_PARAM_GRADS (no_param_grads)": _SKIP_PARAM_GRADS[0],
        "_SKIP_LEAF_INPUT_GRADS (no_leaf_input_grads)": _SKIP_LEAF_INPUT_GRADS[0],
        "FROZEN_CAPTURE (mnk.graphs.frozen_weights)": FROZEN_CAPTURE[0],
    }
    return {k: v for k, v in slots.items() if v}


def pending_outputs():
    """data pointers of convolution outputs that still wait for the norm layer behind them (a deferred split-K launch's partial sums,
    a fused launch's hand-through): a tensor kept across calls must not be among them"""
    return set(_SPLIT_PENDING) | set(_FUSED_PENDING)


# ---- what the running backward pass asked for ---------------------------------------------------------------------------------------
# `ctx.needs_input_grad[i]` of a custom Function says that input i REQUIRES a gradient, not that this pass delivers one:
# torch.autograd.grad(loss, x) and loss.backward(inputs=[x]) run the node with the flag of every parameter still True.  A returned
# gradient nobody asked for is dropped by the engine, but a SIDE EFFECT of computing it -- weight-gradient partials written towards
# an optimiser's sink (DeferredReducer.wgrad) -- stays and is summed into the next step.  The engine knows: inside a backward pass
# torch._C._will_engine_execute_node(node) answers for the node behind input i (a parameter's AccumulateGrad).
_WILL_EXECUTE = getattr(torch._C, "_will_engine_execute_node", None)
GRAD_DELIVERED, GRAD_RETURNED, GRAD_UNWANTED = "delivered", "returned", "unwanted"


def edge_index(args, i):
    """the position of forward argument `i` among the node's edges (`ctx.next_functions`): only tensor arguments have one"""
    return sum(1 for a in args[:i] if torch.is_tensor(a))


def param_grad_request(ctx, edge):
    """What the running backward pass does with the gradient of the parameter behind edge `edge` (edge_index) of the node `ctx`:
    GRAD_DELIVERED  it reaches the parameter (backward(), backward(inputs=[... p ...])): side effects towards a sink are in order;
    GRAD_RETURNED   the parameter itself is an input of torch.autograd.grad(): the caller gets the tensor this node returns and
                    p.grad stays as it is -- the gradient is computed by the per-layer path, nothing is written towards a sink;
    GRAD_UNWANTED   nobody asked (autograd.grad(loss, x), backward(inputs=[x])): no weight / bias gradient work at all.
    A torch without the query keeps GRAD_DELIVERED (the behaviour before the query was used)."""
    if _WILL_EXECUTE is None:
        return GRAD_DELIVERED
    node = ctx.next_functions[edge][0]
    if node is None:
        return GRAD_DELIVERED
    try:
        return GRAD_DELIVERED if _WILL_EXECUTE(node) else GRAD_UNWANTED
    except RuntimeError:
        # "A leaf node was passed to _will_engine_execute_node but we are currently running autograd.grad()"
        return GRAD_RETURNED


def _dgrad_rec(rec, cc, shape):
    """the norm-layer record (_BN_OF) a data-gradient launch into a source of `cc` channels keeps, or None: the record must be of
    that width, and small layers make their backward statistics inside their own one-launch kernel.  shape: what rec.y must look
    like (None: not checked here)"""
    if rec is None:
        return None
    rows = rec.y.numel() // rec.y.shape[-1]
    if rec.c != cc or rec.y.shape[-1] != ceil4(cc) or small_bn(rows, True, cc) or _small_sync(rows):
        return None
    return rec if shape is None or tuple(rec.y.shape) == shape else None


def _up_dgrad_pair(dy, cout, wds, n, h, w, cs, recs):
    """The data gradients of an up-sampled convolution w.r.t. both of its sources as ONE launch (mnk_conv3x3_up_dgrad_pair: the
    two GEMMs read the same dy and keep their own plans, so every bit is that of the two single launches) -> [dx0, dx1], with the
    _DZ_STATS hand-over of each source that has a record; None where the pair is not one launch at this shape and tuning
    (mnk_conv3x3_up_dgrad_pair_form): the caller issues the two launches.  (n, h, w): the low resolution."""
    if dy.shape[-1] != ceil4(cout) or dy.data_ptr() % 16:
        return None
    if not _query("mnk_conv3x3_up_dgrad_pair_form", n, h, w, cout, cs[0], cs[1], int(recs[0] is not None), int(recs[1] is not None)):
        return None
    _drop_stale_split_pending()
    dxs = [torch.empty(n, h, w, ceil4(c), dtype=torch.float32, device=dy.device) for c in cs]
    nws = _query("mnk_conv3x3_up_dgrad_pair_workspace_floats", n, h, w, cout, cs[0], cs[1])
    ws = SCRATCH.get("ws", nws, dy) if nws else None
    head = (_p(dy), dy.shape[-1], cout, _p(wds[0]), _p(wds[1]), _p(dxs[0]), dxs[0].shape[-1], _p(dxs[1]), dxs[1].shape[-1], n, h, w,
            cs[0], cs[1], _p(ws), nws)
    if recs[0] is None and recs[1] is None:
        _call("mnk_conv3x3_up_dgrad_pair", dy, *head)
        return dxs
    sts, tail = [], ()
    for c, rec in zip(cs, recs):
        if rec is None:
            sts.append(None)
            tail += (None, None, 0, None, None, None, None, -1.0)
            continue
        st = torch.empty(_query("mnk_conv3x3_up_dgrad_stats_floats", n, h, w, cout, c), dtype=torch.float32, device=dy.device)
        sts.append(st)                   # lives until the norm layer reads it
        tail += (_p(st), _p(rec.y), rec.y.shape[-1], _p(rec.mean), _p(rec.invstd), _p(rec.scale), _p(rec.beta), float(rec.slope))
    _call("mnk_conv3x3_up_dgrad_pair_bnstats", dy, *head, *tail)
    for dx, st, rec in zip(dxs, sts, recs):
        if st is not None:
            _DZ_STATS[dx.data_ptr()] = (dx, st, st.numel() // (2 * dx.shape[-1]), rec.y.data_ptr(), dx._version)
    return dxs


class Conv3x3Fn(_Fn):
    """nn.Conv3d((1,3,3), padding (0,1,1)) over the channel concatenation [x0 | x1], optionally read through the
    nearest x2 up-sampling (UpBlock3D, modules/util.py:83-85), plus bias and residual add (ResBlock3D :66-67)."""

    @staticmethod
    def forward(ctx, x0, x1, weight, bias, residual, c0, c1, ups, want_stats, track, src_bn=None, eval_defer=False,
                train_bf16=False):
        """src_bn: (the _BnRecord of the norm layer whose output x0 is, or None; the same for x1), see _BN_OF.
        eval_defer: conv3x3(eval_bn=True), see _conv_launch.  train_bf16: conv3x3 was called with gradients enabled inside
        training_precision("bf16")."""
        _check_device(x0)
        cout = weight.shape[0]
        # the node's precision, decided once: its three GEMMs are bf16 or none is
        ctx.bf16 = bool(train_bf16) and not bf16_excluded(c0 + c1, cout)
        assert weight.shape[1] == c0 + c1 and weight.is_contiguous()
        n, hs, ws_, _ = x0.shape
        h, w = (hs * 2, ws_ * 2) if ups else (hs, ws_)
        up = subpixel(ups) and residual is None
        if track:
            # a backward will follow: the parameter changes every step -> packed per iteration (forward + the
            # data-gradient layouts the backward will need), by repack_registered() or one launch here
            need = [bool(cc and ctx.needs_input_grad[i]) for i, cc in enumerate((c0, c1))]
            e = _pack_entry(weight, cout, c0, c1, need, up, dead1x1=up and up1x1_dead_taps(n, hs, ws_))
            wp, ctx.wd = e.wp, list(e.wd)
            ctx.edges = (edge_index((x0, x1, weight), 2), edge_index((x0, x1, weight, bias), 3))      # of weight and bias
        else:
            wp = _packed_fwd_weight(weight, cout, c0, c1, up)
        y, sums = _conv_launch(x0, c0, x1, c1, ups, wp, bias, residual, n, h, w, cout, want_stats, up, eval_defer, ctx.bf16)
        ctx.up = up
        ctx.src_bn = src_bn if track and src_bn is not None else (None, None)
        ctx.save_for_backward(x0, x1, weight)
        ctx.meta = (c0, c1, ups, cout, n, h, w, bias is not None, residual is not None)
        if sums is None:
            sums = y.new_empty(0)
        ctx.mark_non_differentiable(sums)
        ctx.set_materialize_grads(False)     # `sums` never has a gradient: no zero tensor is made for it per backward
        return y, sums

    @staticmethod
    def backward(ctx, dy, _dsums):
        return Conv3x3Fn._backward(ctx, dy, None)

    @staticmethod
    def _backward(ctx, dy, dskip):
        """dskip: a second gradient of x0 (Conv3x3SkipFn: x0's other consumer), added in the data gradient's epilogue."""
        x0, x1, weight = ctx.saved_tensors
        c0, c1, ups, cout, n, h, w, has_bias, has_res = ctx.meta
        if dy is None:                       # (materialize_grads is off) nothing flows into y
            return (dskip if ctx.needs_input_grad[0] else None,) + (None,) * 12
        if dskip is not None and not ctx.needs_input_grad[0]:
            dskip = None
        dy_in = dy
        dy = dy.contiguous()
        ld_dy = dy.shape[-1]
        cin = c0 + c1
        grads = [None, None]
        pair = None
        if ctx.up and not ctx.bf16 and x1 is not None and c1 and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
            # both sources of an up-sampled convolution: the two data gradients read the same dy -- one launch where the library
            # can make them one (else None: the loop below)
            shapes = [(n, h // 2, w // 2, ceil4(cc)) for cc in (c0, c1)]
            pair = _up_dgrad_pair(dy, cout, ctx.wd, n, h // 2, w // 2, (c0, c1),
                                  [_dgrad_rec(ctx.src_bn[i], cc, shapes[i]) for i, cc in enumerate((c0, c1))])
        for i, (src, cs, cc) in enumerate(((x0, 0, c0), (x1, c0, c1))):
            if src is None or not ctx.needs_input_grad[i]:
                continue
            if pair is not None:
                grads[i] = pair[i]
                continue
            wp = ctx.wd[i]                       # packed in the forward (mnk_conv3x3_pack_all)
            # the source is the output of a norm layer (no pooling) and (presumably) has no other consumer: this launch also
            # leaves that layer's backward statistics (see _BN_OF); rows = the geometry both tensors share
            rec = _dgrad_rec(ctx.src_bn[i], cc, None)
            res = None
            if ctx.up:
                # data gradient w.r.t. the low-resolution source: one 4x4 / stride 2 convolution over dy (no gradient of
                # the up-sampled view, no 2x2 sum-pool pass)
                form, hd, wd = "up_dgrad", h // 2, w // 2
            else:
                form, hd, wd = "3x3", h, w
                # x0's second gradient rides as the residual operand of the data-gradient GEMM (its epilogue / split reduction)
                if i == 0 and dskip is not None and not ups:
                    res, dskip = dskip.contiguous(), None
                    assert res.shape == (n, h, w, ceil4(cc))
                if ups:
                    rec = None
            if rec is not None and tuple(rec.y.shape) != (n, hd, wd, ceil4(cc)):
                rec = None
            dx, st = _gemm_launch(form, dy, cout, None, 0, wp, None, res, n, hd, wd, cc, 2 | (16 if ctx.bf16 else 0), bn=rec)
            if rec is not None and st is not None:
                _DZ_STATS[dx.data_ptr()] = (dx, st, st.numel() // (2 * dx.shape[-1]), rec.y.data_ptr(), dx._version)
            if ups and not ctx.up:
                dxs = torch.empty(n, h // 2, w // 2, ceil4(cc), dtype=torch.float32, device=dy.device)
                _call("mnk_sumpool2x2", dy, _p(dx), dx.shape[-1], _p(dxs), dxs.shape[-1], n, h, w, cc)
                dx = dxs
            grads[i] = dx
        dw = None
        want_w = param_grad_request(ctx, ctx.edges[0]) if ctx.needs_input_grad[2] else GRAD_UNWANTED
        if want_w != GRAD_UNWANTED:
            # an optimiser of mnk.optim owns this parameter: the GEMM writes (the partials of) its gradient towards the
            # optimiser's flat buffer and the split reduction waits for the one launch that serves every layer
            # (GRAD_RETURNED: the caller of torch.autograd.grad gets dW itself, the sink is left alone)
            owner = wgrad_sink_owner(weight) if want_w == GRAD_DELIVERED else None
            taken = [False, False]
            # | 2: MNK_CONV_CLEAN_PADS (x and dy are acts of this module); | 8: MNK_WGRAD_BF16, the precision the forward recorded
            wflags = int(ups) | 2 | (8 if ctx.bf16 else 0)
            if owner is not None:
                for i, (src, cs, cc) in enumerate(((x0, 0, c0), (x1, c0, c1))):
                    if src is not None:
                        taken[i] = owner.reducer.wgrad(weight, src, src.shape[-1], cc, wflags, h, w, 3, 3, 1, dy,
                                                       ld_dy, cout, cin, cs, n, h, w)
            rest = [(src, cs, cc) for i, (src, cs, cc) in enumerate(((x0, 0, c0), (x1, c0, c1)))
                    if src is not None and not taken[i]]
            if rest:
                dw = torch.zeros_like(weight) if len(rest) < (1 + (x1 is not None)) else torch.empty_like(weight)
            for src, cs, cc in rest:
                nws = _query("mnk_conv3x3_up_wgrad_workspace_floats" if ups else "mnk_conv3x3_wgrad_workspace_floats", n, h, w,
                             cc, cout)
                ws = SCRATCH.get("ws", nws, dy) if nws else None
                _call("mnk_conv3x3_wgrad", dy, _p(src), src.shape[-1], cc, wflags, _p(dy), ld_dy, cout, _p(dw), cin,
                      cs, n, h, w, _p(ws), nws)
            if owner is not None and dw is not None:
                owner.add_to_sink(weight, dw)        # a further contribution before the step (slow path)
                dw = None
        db = None
        # the slot is one-shot: whatever the norm layer behind this convolution left is taken here, bias or no bias (a frozen or
        # absent bias would otherwise leave a dy-sized tensor pinned until the next norm layer's backward)
        slot, _DY_SUMS[0] = _DY_SUMS[0], None
        if has_bias and ctx.needs_input_grad[3] and param_grad_request(ctx, ctx.edges[1]) != GRAD_UNWANTED:
            if slot is not None and slot[0] is dy_in and slot[1] is None:
                db = None                      # a training-mode BatchNorm follows: the bias gradient is exactly zero
            elif slot is not None and slot[0] is dy_in and slot[1].numel() == cout:
                db = slot[1]                   # column sums of dy came out of the norm layer's backward pass
            else:
                db = channel_sums(dy, cout)[:cout]
        dres = dy if has_res and ctx.needs_input_grad[4] else None
        if dskip is not None:                # forms without a residual operand (up-sampled sources): one add
            grads[0] = grads[0] + dskip if grads[0] is not None else dskip
        return grads[0], grads[1], dw, db, dres, None, None, None, None, None, None, None, None


class Conv3x3SkipFn(_Fn):
    """Conv3x3Fn that also hands x0 through: -> (y, sums, x0).  For a tensor with a second consumer (an hourglass level:
    the next down block's convolution AND the decoder's skip / a warp, util.py:142-152,184-188) the second consumer takes
    the handed-through tensor; this node is then the only consumer of the original and its backward adds the other
    gradient in the epilogue of its data-gradient GEMM (the `residual` operand) -- no accumulation pass by autograd."""

    @staticmethod
    def forward(ctx, x0, x1, weight, bias, residual, c0, c1, ups, want_stats, track, src_bn=None, eval_defer=False,
                train_bf16=False):
        y, sums = Conv3x3Fn.forward(ctx, x0, x1, weight, bias, residual, c0, c1, ups, want_stats, track, src_bn, eval_defer,
                                    train_bf16)
        return y, sums, x0

    @staticmethod
    def backward(ctx, dy, _dsums, dskip):
        return Conv3x3Fn._backward(ctx, dy, dskip)


# ---- opt-in evaluation-mode norm fusion --------------------------------------------------------------------------------------
# In evaluation mode the norm layer behind a convolution is a constant per-channel affine.  Inside `eval_norm_fusion(True)` an
# UNSPLIT 3x3 / sub-pixel forward launched under torch.no_grad() for a caller that vouches for its norm layer (conv3x3(eval_bn=True,
# follow=(norm, relu, pool))) applies that layer, its ReLU and (DownBlock3D) the 2x2 average pool in its own epilogue
# (mnk_conv3x3_fwd_evalnorm / mnk_conv3x3_up_fwd_evalnorm): z is written once and y never.  Equal to the two launches bit for bit.
# Where the library's form query answers 0 -- a split plan (the deferred-split hand-over serves it), a pooled layer without a
# window-major kernel -- and in training, with gradients enabled or with the scope off, everything is what it was.
# the finished output of a fused launch on its way to the bn_act that the caller runs next: z.data_ptr() -> (z, norm, relu, pool)
_FUSED_PENDING = {}
# conv -> evaluation-mode norm pairs (callers that pass `follow`) under no_grad since clear_eval_norm_count():
# [fused per element, fused with the pool, deferred split-K (mnk_bn_eval_split_fwd), separate launches]
EVAL_NORM_COUNT = [0, 0, 0, 0]
_PAIR_PENDING = [None]                    # y.data_ptr() of an unfused pair's convolution, for the count in bn_act


def eval_norm_fusion(on=True):
    """Context manager: `with eval_norm_fusion(True):` (see above) -- eval_options with this one field."""
    return eval_options(fuse_norm=bool(on))


def current_norm_fusion():
    return _EVAL.fuse_norm


def clear_eval_norm_count():
    EVAL_NORM_COUNT[:] = [0, 0, 0, 0]


def _conv_evalnorm(x0, c0, x1, c1, ups, weight, bias, norm, relu, pool):
    """conv3x3's fused evaluation form: -> z = pool(act(norm(conv))) from one launch, or None where the form query answers 0 (or
    the sources are not laid out as the query assumes): the caller then takes the ordinary path."""
    cout = weight.shape[0]
    if norm.weight is None or norm.bias is None or norm.running_mean is None or norm.weight.shape[0] != cout:
        return None
    _check_device(x0)
    for t, c in ((x0, c0), (x1, c1)):
        if t is not None and (t.shape[-1] != ceil4(c) or t.data_ptr() % 16 or not t.is_contiguous()):
            return None
    n, hs, ws_, _ = x0.shape
    h, w = (hs * 2, ws_ * 2) if ups else (hs, ws_)
    up = subpixel(ups)
    if pool and (up or h % 2 or w % 2):
        return None
    hq, wq, flags = _fwd_launch_geometry(ups, up, h, w, c0, c1, cout)
    form = _query("mnk_conv3x3_evalnorm_form", n, hq, wq, c0, c1, cout, flags, int(up), int(pool))
    if not form:
        return None
    if _FUSED_PENDING:
        import warnings
        warnings.warn("dropping the output of %d fused convolution(s) whose norm layer never asked for it (an exception between "
                      "a convolution and its normalisation layer?)" % len(_FUSED_PENDING))
        _FUSED_PENDING.clear()
    wp = _packed_fwd_weight(weight, cout, c0, c1, up)
    mean, _invstd, scale = _bn_eval_coeffs(x0, norm.weight, norm.running_mean, norm.running_var, norm.eps, cout)
    z = torch.empty(n, h // 2 if pool else h, w // 2 if pool else w, ceil4(cout), dtype=torch.float32, device=x0.device)
    ld1 = x1.shape[-1] if x1 is not None else 0
    head = (x0, _p(x0), x0.shape[-1], c0, _p(x1), ld1, c1, flags, _p(wp), _p(bias), _p(mean), _p(scale), _p(norm.bias), int(relu))
    if up:
        _call("mnk_conv3x3_up_fwd_evalnorm", *head, _p(z), z.shape[-1], n, hq, wq, cout)
    else:
        _call("mnk_conv3x3_fwd_evalnorm", *head, int(pool), _p(z), z.shape[-1], n, h, w, cout)
    EVAL_NORM_COUNT[form - 1] += 1
    _FUSED_PENDING[z.data_ptr()] = (z, norm, bool(relu), bool(pool))
    return z


# ---- opt-in weight-streaming ("skinny") convolutions for batch-1 evaluation ---------------------------------------------------
# Inside `eval_skinny_conv(True)` a 3x3 or up-sampled 3x3 convolution launched under torch.no_grad() for a caller that vouches for
# its evaluation-mode norm layer (conv3x3(eval_bn=True, follow=...)) and whose output has few rows (mnk_conv3x3_skinny_form: at
# most "skinny_rows") runs as mnk_conv3x3_skinny_fwd on a pack of its own (plain nine taps, bf16 elements under
# inference_precision("bf16")) and leaves split partials to the norm layer through the deferred split-K hand-over
# (_SPLIT_PENDING -> mnk_bn_eval_split_fwd).  With gradients enabled, in training, or with the scope off nothing changes.
EVAL_SKINNY_COUNT = [0]                   # layers that took the form since clear_eval_skinny_count()


def eval_skinny_conv(on=True):
    """Context manager: `with eval_skinny_conv(True):` (see above) -- eval_options with this one field."""
    return eval_options(skinny=bool(on))


def current_skinny_conv():
    return _EVAL.skinny


def clear_eval_skinny_count():
    EVAL_SKINNY_COUNT[0] = 0


def _packed_skinny_weight(weight, cout, c0, c1, bf16):
    """The skinny pack of a conv weight (mnk_conv3x3_skinny_pack; bf16: half the bytes), cached by _cached_pack per precision."""
    nfloats = _query("mnk_conv3x3_skinny_packed_floats", cout, c0, c1, int(bf16))
    return _cached_pack(("skinny", bool(bf16)), weight, (cout, c0, c1), nfloats,
                        lambda wp: _call("mnk_conv3x3_skinny_pack", weight, _p(weight), _p(wp), cout, c0, c1, int(bf16)))


def _conv_skinny(x0, c0, x1, c1, ups, weight, bias, norm, relu, pool):
    """conv3x3's weight-streaming form: -> y, a handle that is never written, whose partials wait in _SPLIT_PENDING for the bn_act
    the caller runs next; or None where the form query answers 0: the caller then takes the ordinary path."""
    cout = weight.shape[0]
    _check_device(x0)
    for t in (x0, x1):
        if t is not None and not t.is_contiguous():
            return None
    n, hs, ws_, _ = x0.shape
    h, w = (hs * 2, ws_ * 2) if ups else (hs, ws_)
    if h % 2 or w % 2:                       # the hand-over's condition (BNActFn.forward)
        return None
    _, _, flags = _fwd_launch_geometry(ups, False, h, w, c0, c1, cout)       # never the sub-pixel form: the full resolution
    if not _query("mnk_conv3x3_skinny_form", n, h, w, c0, c1, cout, flags, int(bool(pool))):
        return None
    _drop_stale_split_pending()
    wp = _packed_skinny_weight(weight, cout, c0, c1, bool(flags & 8))
    size = (n, h, w, c0, c1, cout)
    nws = _query("mnk_conv3x3_skinny_workspace_floats", *size)
    ws = SCRATCH.get("ws", nws, x0)
    y = torch.empty(n, h, w, ceil4(cout), dtype=torch.float32, device=x0.device)
    _call("mnk_conv3x3_skinny_fwd", x0, _p(x0), x0.shape[-1], c0, _p(x1), x1.shape[-1] if x1 is not None else 0, c1, flags, _p(wp),
          n, h, w, cout, _p(ws), nws)
    _SPLIT_PENDING[y.data_ptr()] = _SplitPending(ws, _query("mnk_conv3x3_skinny_splits", *size), 1, bias)
    EVAL_SKINNY_COUNT[0] += 1
    return y


def conv3x3(x0, c0, weight, bias=None, x1=None, c1=0, ups=False, residual=None, want_stats=False, skip=False, eval_bn=False,
            follow=None):
    """-> (y, sums): sums = fused BatchNorm statistics [sum, sum of squares] of y when want_stats, else None.
    skip: -> (y, sums, x0 handed through for x0's other consumer), see Conv3x3SkipFn.
    eval_bn: the caller vouches that y's ONLY consumer is the evaluation-mode norm layer it calls next (bn_act): under no_grad a
    split-K launch then leaves its partials to that layer (mnk_bn_eval_split_fwd: reduction + affine + ReLU + pool in one launch)
    and y is never written.
    follow: (norm, relu, pool) of that bn_act call.  Inside eval_norm_fusion(True) an unsplit launch then applies the layer itself
    and what comes back as `y` is the finished z: the bn_act that follows recognises it and hands it through."""
    if _EVAL.precision != "fp32":
        if torch.is_grad_enabled():
            raise RuntimeError("a convolution with gradients enabled inside inference_precision(%r): the backward kernels are "
                               "fp32 and would not differentiate what was computed -- call it under torch.no_grad()" % _EVAL.precision)
        if want_stats:
            raise RuntimeError("inference_precision(%r) is for evaluation-mode networks: a training-mode norm layer asked this "
                               "convolution for batch statistics" % _EVAL.precision)
    track = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (x0, x1, weight, bias, residual))
    eval_defer = bool(eval_bn and not want_stats and residual is None and not torch.is_grad_enabled()
                      and knobs.form("EVAL_SPLIT_FUSED"))
    pair = eval_defer and follow is not None and not follow[0].training
    if pair and _EVAL.skinny:
        # few output rows: the weight-streaming launch; its partials go to the norm layer like a deferred split-K launch's
        y = _conv_skinny(x0, c0, x1, c1, ups, weight, bias, *follow)
        if y is not None:
            _PAIR_PENDING[0] = y.data_ptr()
            return (y, None, x0) if skip else (y, None)
    if pair and _EVAL.fuse_norm:
        # a conv -> evaluation-mode norm pair under no_grad: fused where the scope is on and the library has the form
        z = _conv_evalnorm(x0, c0, x1, c1, ups, weight, bias, *follow)
        if z is not None:
            return (z, None, x0) if skip else (z, None)
    src_bn = (_bn_of(x0), _bn_of(x1)) if track else None     # the norm layers whose outputs the sources are (see _BN_OF)
    # training_precision("bf16"): a call with gradients enabled; no_grad calls are left to inference_precision
    train_bf16 = _TRAIN_PRECISION[0] == "bf16" and torch.is_grad_enabled()
    args = (x0, x1, weight, bias, residual, c0, c1, bool(ups), bool(want_stats), track, src_bn, eval_defer, train_bf16)
    if skip and track and x0.requires_grad and knobs.form("SKIP_GRAD_FUSED"):
        y, sums, through = Conv3x3SkipFn.apply(*args)
        return y, (sums if want_stats else None), through
    y, sums = Conv3x3Fn.apply(*args)
    if pair:
        _PAIR_PENDING[0] = y.data_ptr()      # bn_act counts the pair: deferred split-K or separate launches (EVAL_NORM_COUNT)
    return (y, (sums if want_stats else None), x0) if skip else (y, (sums if want_stats else None))


# ----------------------------------------------------------------------------------------------------------------
# BatchNorm (+ReLU, +2x2 average pool)
# ----------------------------------------------------------------------------------------------------------------
# Evaluation-mode coefficients (mean, 1/sqrt(var + eps), gamma / sqrt(var + eps)) of a norm layer, kept between calls: the
# reference's evaluation loops run the networks frame by frame with constant weights, and the coefficient launch was 40 of
# the 135 launches per frame (tools/frame_loop_probe.py).  Valid while nothing wrote the layer's tensors: tensor versions
# (load_state_dict, in-place ops), storage addresses, the optimiser-step / replay epoch (_PACK_EPOCH: fused optimisers and
# captured iterations do not bump versions) and the training-forward epoch (kernels update running statistics through raw
# pointers) are all part of the key; never used under stream capture (a replay must read the live buffers).
_BN_EVAL = {}
_BN_EVAL_EPOCH = [0]


def _bn_eval_coeffs(y, gamma, running_mean, running_var, eps, c):
    capturing = y.is_cuda and torch.cuda.is_current_stream_capturing() and not FROZEN_CAPTURE[0]
    if not capturing:
        key = (0 if gamma is None else gamma.data_ptr(), 0 if gamma is None else gamma._version, running_mean.data_ptr(),
               running_mean._version, running_var.data_ptr(), running_var._version, float(eps), c, _stream(y),
               _PACK_EPOCH[0], _BN_EVAL_EPOCH[0])
        hit = _BN_EVAL.get(id(running_mean))
        if hit is not None and hit[0] == key and hit[2]() is running_mean:
            return hit[1]
    mean = torch.empty(c, dtype=torch.float32, device=y.device)
    invstd, scale = torch.empty_like(mean), torch.empty_like(mean)
    _call("mnk_bn_eval_coeffs", y, _p(gamma), _p(running_mean), _p(running_var), float(eps), c, _p(mean), _p(invstd), _p(scale))
    if not capturing:
        if id(running_mean) not in _BN_EVAL:
            weakref.finalize(running_mean, _BN_EVAL.pop, id(running_mean), None)
        _BN_EVAL[id(running_mean)] = (key, (mean, invstd, scale), weakref.ref(running_mean))
    return mean, invstd, scale


class BNActFn(_Fn):
    """SynchronizedBatchNorm3d (sync_batchnorm/batchnorm.py:48-78) fused with the ReLU and the AvgPool3d((1,2,2))
    that follow it in DownBlock3D / UpBlock3D / SameBlock3D / ResBlock3D (modules/util.py).  In training mode under
    torch.distributed the sufficient statistics are all-reduced over the ranks (SyncBN over RCCL)."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, pre_sums, c, training, relu, pool, momentum, eps):
        _check_device(y)
        n, h, w, ld = y.shape
        rows = n * h * w
        dev = y.device
        if training:
            _BN_EVAL_EPOCH[0] += 1          # kernels are about to write running statistics through raw pointers
        if training:
            mean = torch.empty(c, dtype=torch.float32, device=dev)
            invstd = torch.empty_like(mean)
            scale = torch.empty_like(mean)
        count = float(rows)
        pending = _SPLIT_PENDING.pop(y.data_ptr(), None)
        ctx.small = False
        ho, wo = (h // 2, w // 2) if pool else (h, w)
        z = torch.empty(n, ho, wo, ceil4(c), dtype=torch.float32, device=dev)     # every kernel zeroes the pad channels
        if small_bn(rows, training, c) and ld == ceil4(c) and h % (2 if pool else 1) == 0 and w % (2 if pool else 1) == 0:
            # the whole layer in one launch (csrc/batchnorm.hip: bn_small_fwd_kernel; several ranks: bn_small_fwd_sync_kernel,
            # the exchange of the sums inside the launch, statistics over the rows of ALL ranks)
            sp = pending if pending is not None else _NO_SPLIT
            if mdist.active():
                count *= mdist.world_size()
                _call("mnk_bn_small_fwd_sync", y, _sync_handle(c), _p(sp.ws), sp.splits, ld, sp.phases, _p(sp.bias), _p(y), ld, n, h, w, c,
                      _p(gamma), _p(beta), _p(running_mean), _p(running_var), float(momentum), float(eps), _p(mean), _p(invstd),
                      _p(scale), _p(z), z.shape[-1], int(relu), int(pool), mdist.P2P_TIMEOUT_MS)
            else:
                _call("mnk_bn_small_fwd", y, _p(sp.ws), sp.splits, ld, sp.phases, _p(sp.bias), _p(y), ld, n, h, w, c, _p(gamma), _p(beta),
                      _p(running_mean), _p(running_var), float(momentum), float(eps), _p(mean), _p(invstd), _p(scale), _p(z),
                      z.shape[-1], int(relu), int(pool))
            ctx.save_for_backward(y, mean, invstd, scale, beta)
            ctx.meta = (c, training, relu, pool, count)
            ctx.small = True
            return z
        if pending is not None and not training and ld == ceil4(c) and h % 2 == 0 and w % 2 == 0:
            # evaluation mode behind a split-K convolution (conv3x3(eval_bn=True), no_grad): reduction + affine + ReLU + pool in
            # one launch; y was never written and nothing is saved for a backward pass
            mean, invstd, scale = _bn_eval_coeffs(y, gamma, running_mean, running_var, eps, c)
            _call("mnk_bn_eval_split_fwd", y, _p(pending.ws), pending.splits, ld, pending.phases, _p(pending.bias), _p(mean), _p(scale), _p(beta), _p(z),
                  z.shape[-1], n, h, w, c, int(relu), int(pool))
            return z
        if pending is not None:
            raise RuntimeError("split-K partials were deferred to a BatchNorm that does not take the small-layer path")
        if training:
            if rows * mdist.world_size() <= 1:
                raise ValueError("BatchNorm needs more than one value per channel in training mode "
                                 "(sync_batchnorm/batchnorm.py:116)")
            if mdist.active():
                sums = pre_sums if pre_sums is not None and pre_sums.numel() == 2 * c else channel_sums(y, c, sync=True)
                if _take_reduced(sums):                  # the statistics' second stage carried the exchange
                    pass
                else:
                    sums = mdist.all_reduce_sum(sums) if sums is pre_sums else mdist.all_reduce_sum_(sums)
                count *= mdist.world_size()
                # finalisation inside the apply pass (mnk_bn_act_fwd_sums): one launch less per norm layer on the SyncBN path
                _call("mnk_bn_act_fwd_sums", y, _p(y), ld, _p(sums), count, _p(gamma), _p(beta), _p(running_mean),
                      _p(running_var), float(momentum), float(eps), 1, _p(mean), _p(invstd), _p(scale), _p(z), z.shape[-1], 0, n, h,
                      w, c, int(relu), int(pool))
                ctx.save_for_backward(y, mean, invstd, scale, beta)
                ctx.meta = (c, training, relu, pool, count)
                if not pool and ld == z.shape[-1] and knobs.form("DGRAD_BN_STATS"):
                    _LAST_BN[0] = _BnRecord(y, mean, invstd, scale, beta, c, 0.0 if relu else -1.0)
                return z
            else:
                # one launch for second stage + finalisation; partials from the conv epilogue when it produced them
                part = pre_sums if pre_sums is not None and pre_sums.numel() > 2 * c else None
                if pre_sums is not None and part is None and pre_sums.numel() == 2 * c:
                    _call("mnk_bn_finalize", y, _p(pre_sums), count, _p(gamma), _p(running_mean), _p(running_var),
                          float(momentum), float(eps), c, 1, _p(mean), _p(invstd), _p(scale))
                else:
                    nws = 0 if part is not None else _query("mnk_bn_workspace_floats", rows, ld)
                    ws = SCRATCH.get("ws", nws, y) if nws else None
                    _call("mnk_bn_stats_finalize", y, _p(y), ld, rows, c, _p(part),
                          part.numel() // (2 * ld) if part is not None else 0, count, _p(gamma), _p(running_mean),
                          _p(running_var), float(momentum), float(eps), 1, None, _p(mean), _p(invstd), _p(scale),
                          _p(ws), nws)
        else:
            mean, invstd, scale = _bn_eval_coeffs(y, gamma, running_mean, running_var, eps, c)
        _call("mnk_bn_act_fwd", y, _p(y), ld, _p(mean), _p(scale), _p(beta), _p(z), z.shape[-1], 0, n, h, w, c, int(relu),
              int(pool))
        ctx.save_for_backward(y, mean, invstd, scale, beta)
        ctx.meta = (c, training, relu, pool, count)
        if training and not pool and ld == z.shape[-1] and knobs.form("DGRAD_BN_STATS"):
            _LAST_BN[0] = _BnRecord(y, mean, invstd, scale, beta, c, 0.0 if relu else -1.0)
        return z

    @staticmethod
    def backward(ctx, dz):
        return BNActFn._backward(ctx, dz, None)

    @staticmethod
    def _backward(ctx, dz, dskip):
        """dskip: a second gradient of y (BNActSkipFn: the skip path of a residual block), added inside the dy pass."""
        y, mean, invstd, scale, beta = ctx.saved_tensors
        c, training, relu, pool, count = ctx.meta
        dz = dz.contiguous()
        n, h, w, ld = y.shape
        rows = n * h * w
        if dskip is not None:
            dskip = dskip.contiguous()
            assert dskip.shape == y.shape, "the skip gradient of a residual block has the shape of the block's input"
        # a small layer: statistics, (several ranks: their exchange inside the launch,) and the apply pass in ONE launch
        # (mnk_bn_small_bwd / mnk_bn_small_bwd_sync) -- the general path spends three to four launches here
        sync = None
        small = ctx.small and not mdist.active()
        if not small:
            sync = _sync_handle(c) if training else None  # several ranks: the second stage carries the exchange of the sums
            small = (sync is not None and _small_sync(rows) and ld == ceil4(c) and 2 * c <= mdist._P2P["max"]
                     and (not pool or (h % 2 == 0 and w % 2 == 0)))
        if small:
            sums = torch.empty(2 * c, dtype=torch.float32, device=y.device)      # this rank's own: [dbeta | dgamma]
            dy = torch.empty(n, h, w, ld, dtype=torch.float32, device=y.device)
            args = (_p(y), ld, _p(dz), dz.shape[-1], _p(mean), _p(invstd), _p(scale), _p(beta), count, n, h, w, c, int(relu),
                    int(pool), _p(sums), _p(dy), ld)
            if sync is None:
                _call("mnk_bn_small_bwd", y, *args)
            else:
                _DZ_STATS.pop(dz.data_ptr(), None)
                _call("mnk_bn_small_bwd_sync", y, sync, *args, mdist.P2P_TIMEOUT_MS)
            if dskip is not None:
                dy = dy + dskip                # few-pixel layers: the one-launch kernel has no addend operand
                _DY_SUMS[0] = None             # ... and the sum's column sums are not zero: the convolution in front makes them
            else:
                _DY_SUMS[0] = (dy, None)
            return dy, sums[c:], sums[:c], None, None, None, None, None, None, None, None, None
        nws = _query("mnk_bn_workspace_floats", rows, ceil4(c))
        ws = SCRATCH.get("ws", nws, y)
        sums = torch.empty(2 * c, dtype=torch.float32, device=y.device)
        pre = _DZ_STATS.pop(dz.data_ptr(), None)
        local = torch.empty(2 * c, dtype=torch.float32, device=y.device) if sync is not None else sums
        if pre is not None and pre[0].shape == dz.shape and pre[3] == y.data_ptr() and not pool and pre[0]._version == pre[4]:
            # this gradient is the data-gradient GEMM's own output: its epilogue left the statistics' first stage
            # (the version: an in-place gradient hook -- z.register_hook(lambda g: g.mul_(2)) -- keeps the address and changes dz)
            if sync is not None:
                _call("mnk_bn_stats_finish_sync", y, sync, _p(pre[1]), pre[2], ld, c, _p(local), _p(sums), mdist.P2P_TIMEOUT_MS)
            else:
                _call("mnk_bn_stats_finish", y, _p(pre[1]), pre[2], ld, c, _p(sums))
            DZ_STATS_COUNT[0] += 1
        else:
            DZ_STATS_COUNT[1] += 1
            if sync is not None:
                _call("mnk_bn_act_bwd_stats_sync", y, sync, _p(y), ld, _p(dz), dz.shape[-1], 0, _p(mean), _p(invstd), _p(scale),
                      _p(beta), n, h, w, c, int(relu), int(pool), _p(local), _p(sums), _p(ws), nws, mdist.P2P_TIMEOUT_MS)
            else:
                _call("mnk_bn_act_bwd_stats", y, _p(y), ld, _p(dz), dz.shape[-1], 0, _p(mean), _p(invstd), _p(scale), _p(beta), n,
                      h, w, c, int(relu), int(pool), _p(sums), _p(ws), nws)
        dbeta, dgamma = local[:c], local[c:]     # local contributions (averaged later together with all gradients)
        if training and mdist.active() and sync is None:
            sums = mdist.all_reduce_sum(sums)
        dy = torch.empty(n, h, w, ld, dtype=torch.float32, device=y.device)
        if dskip is not None:
            # dy = BatchNorm backward + skip gradient in one pass, with the column sums of the SUM: the bias gradient of the
            # convolution that produced y (the previous residual block's second convolution) -- not zero here
            dy_sums = torch.empty(c, dtype=torch.float32, device=y.device)
            _call("mnk_bn_act_bwd_apply_add_colsum", y, _p(y), ld, _p(dz), dz.shape[-1], 0, _p(mean), _p(invstd), _p(scale),
                  _p(beta), _p(sums), count, int(training), _p(dskip), dskip.shape[-1], _p(dy), ld, n, h, w, c, int(relu),
                  int(pool), _p(dy_sums), _p(ws), nws)
            _DY_SUMS[0] = (dy, dy_sums)
        elif training:
            # training-mode statistics: sum over pixels of dy = scale * (sum g - N * mean(g) - k2 * sum xhat) == 0 exactly, so
            # the bias gradient of the convolution in front (util.py:54-56,80-81,99-100) is analytically zero; the reference
            # computes its rounding noise.  No reduction is spent on it: that bias simply receives no gradient (an optimiser
            # then leaves it alone -- BatchNorm cancels any bias anyway).  MNK_BN_ZERO_BIAS_GRAD=0 computes the noise.
            _call("mnk_bn_act_bwd_apply", y, _p(y), ld, _p(dz), dz.shape[-1], 0, _p(mean), _p(invstd), _p(scale), _p(beta),
                  _p(sums), count, 1, _p(dy), ld, n, h, w, c, int(relu), int(pool))
            _DY_SUMS[0] = (dy, None)
        else:
            dy_sums = torch.empty(c, dtype=torch.float32, device=y.device)
            _call("mnk_bn_act_bwd_apply_colsum", y, _p(y), ld, _p(dz), dz.shape[-1], 0, _p(mean), _p(invstd), _p(scale),
                  _p(beta), _p(sums), count, int(training), _p(dy), ld, n, h, w, c, int(relu), int(pool), _p(dy_sums), _p(ws),
                  nws)
            _DY_SUMS[0] = (dy, dy_sums)      # picked up by Conv3x3Fn.backward when it receives this very tensor
        return dy, dgamma, dbeta, None, None, None, None, None, None, None, None, None


class BNActSkipFn(_Fn):
    """BNActFn for the first norm layer of a residual block (util.py:58-67): returns (z, y) -- y handed through for the
    block's `out += x`.  Both consumers of the block's input are then this one node, and its backward adds the gradient of
    the skip path inside the BatchNorm dy pass (mnk_bn_act_bwd_apply_add_colsum) instead of leaving a separate accumulation
    pass over both gradients to autograd."""

    @staticmethod
    def forward(ctx, y, gamma, beta, running_mean, running_var, pre_sums, c, training, relu, pool, momentum, eps):
        z = BNActFn.forward(ctx, y, gamma, beta, running_mean, running_var, pre_sums, c, training, relu, pool, momentum, eps)
        return z, y

    @staticmethod
    def backward(ctx, dz, dskip):
        if dz is None:          # only the skip path was used
            return (dskip,) + (None,) * 11
        return BNActFn._backward(ctx, dz, dskip)


def bn_act(y, c, norm, relu=True, pool=False, sums=None, skip=False):
    """`norm` is a sync_batchnorm.SynchronizedBatchNorm3d parameter holder; `sums` = statistics of y that a conv
    epilogue already produced (training mode).  skip: -> (z, y handed through for a residual add), see BNActSkipFn."""
    if _FUSED_PENDING:
        # y is the finished z of a fused convolution (conv3x3(follow=...) inside eval_norm_fusion): hand it through
        done = _FUSED_PENDING.pop(y.data_ptr(), None)
        if done is not None:
            if done[0] is not y or done[1] is not norm or done[2:] != (bool(relu), bool(pool)) or skip or y.shape[-1] != ceil4(c):
                raise RuntimeError("a convolution applied the norm layer its caller announced (conv3x3(follow=...)), and another "
                                   "bn_act call followed it")
            return y
    pair, _PAIR_PENDING[0] = _PAIR_PENDING[0], None
    if pair is not None and pair == y.data_ptr() and not norm.training and not torch.is_grad_enabled():
        EVAL_NORM_COUNT[2 if pair in _SPLIT_PENDING else 3] += 1
    fn = BNActSkipFn if skip and knobs.form("RES_SKIP_FUSED") else BNActFn
    _LAST_BN[0] = None
    out = fn.apply(y, norm.weight, norm.bias, norm.running_mean, norm.running_var,
                   sums if norm.training else None, c, norm.training, relu, pool, norm.momentum, norm.eps)
    rec, _LAST_BN[0] = _LAST_BN[0], None
    if rec is not None and torch.is_grad_enabled():
        z = out[0] if isinstance(out, tuple) else out
        if z.requires_grad:
            _bind_bn(z, rec)
    return (out, y) if skip and fn is BNActFn else out


# ----------------------------------------------------------------------------------------------------------------
# grouped 1x1 conv, 1x1 conv + sigmoid
# ----------------------------------------------------------------------------------------------------------------
_SKIP_PARAM_GRADS = [False]


class no_param_grads:
    """Context: backward passes of the discriminator's convolutions skip their weight / bias gradients (the caller
    asked torch.autograd.grad for input gradients only -- a custom Function cannot see that restriction)."""

    def __enter__(self):
        self.prev, _SKIP_PARAM_GRADS[0] = _SKIP_PARAM_GRADS[0], True

    def __exit__(self, *exc):
        _SKIP_PARAM_GRADS[0] = self.prev


_SKIP_LEAF_INPUT_GRADS = [False]


class no_leaf_input_grads:
    """Context: a ConvKxKFn marked `leaf_input` (the discriminator's first convolution) skips its data gradient -- the
    caller's backward only asks for parameter gradients and nothing below that convolution will run (the custom
    Function cannot see torch.autograd.backward(inputs=...))."""

    def __enter__(self):
        self.prev, _SKIP_LEAF_INPUT_GRADS[0] = _SKIP_LEAF_INPUT_GRADS[0], True

    def __exit__(self, *exc):
        _SKIP_LEAF_INPUT_GRADS[0] = self.prev


class ConvKxKFn(_Fn):
    """nn.Conv3d((1,k,k)), stride 1, zero padding `pad`, single source -- the discriminator's 4x4 convolutions without
    padding (modules/discriminator.py:17-18,28) on the same implicit-GEMM kernels; the data gradient is the same
    kernel on dy with pad k-1-pad and the flipped / transposed pack."""

    @staticmethod
    def forward(ctx, x, weight, bias, cin, kh, kw, pad, leaf_input=False):
        _check_device(x)
        ctx.leaf_input = bool(leaf_input)
        cout = weight.shape[0]
        n, hi, wi, ld = x.shape
        ho, wo = hi + 2 * pad - kh + 1, wi + 2 * pad - kw + 1
        nt = kh * kw
        form = _FORMS["kxk"]
        ctx.wd = None
        if nt <= 16 and nt != 9 and weight.requires_grad and weight.is_contiguous():
            # a training forward: the registry entry of the weight (forward and data-gradient layouts: written by the
            # optimiser kernel after its update, else packed here in ONE launch); the data-gradient layout serves every backward
            # pass through this node (the generator pass and the discriminator pass of one iteration read the same, not yet
            # updated, weights)
            e = _pack_entry(weight, cout, cin, 0, [bool(ctx.needs_input_grad[0]), False], ntaps=nt)
            wp, ctx.wd = e.wp, e.wd[0]
        elif ctx.needs_input_grad[0] and nt <= 16:
            wp = SCRATCH.get("pack", _query(form.packed, cout, cin, 0, nt), x)
            ctx.wd = torch.empty(_query(form.packed, cin, cout, 0, nt), dtype=torch.float32, device=x.device)
            _call("mnk_conv2d_pack_all", x, _p(weight), _p(wp), _p(ctx.wd), None, cout, cin, 0, nt)
        else:
            wp = SCRATCH.get("pack", _query(form.packed, cout, cin, 0, nt), x)
            _call(form.pack, x, _p(weight), _p(wp), cout, cin, 0, nt)
        # flags = MNK_CONV_CLEAN_PADS: x is an act of this module (zero pad channels) -> the K x K buffer-load loader
        y, _ = _gemm_launch("kxk", x, cin, None, 0, wp, bias, None, n, ho, wo, cout, 2, kxk=(hi, wi, kh, kw, pad))
        ctx.save_for_backward(x, weight)
        ctx.meta = (cin, cout, kh, kw, pad, n, hi, wi, ho, wo, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        cin, cout, kh, kw, pad, n, hi, wi, ho, wo, has_bias = ctx.meta
        dy = dy.contiguous()
        nt = kh * kw
        dx = dw = db = None
        if ctx.needs_input_grad[0] and not (ctx.leaf_input and _SKIP_LEAF_INPUT_GRADS[0]):
            wp = ctx.wd
            if wp is None:
                wp = SCRATCH.get("pack", _query(_FORMS["kxk"].packed, cin, cout, 0, nt), dy)
                _call("mnk_conv2d_pack_dgrad", dy, _p(weight), _p(wp), cout, cin, 0, cin, nt)
            dx, _ = _gemm_launch("kxk", dy, cout, None, 0, wp, None, None, n, hi, wi, cin, 2, kxk=(ho, wo, kh, kw, kh - 1 - pad))
        want_w = param_grad_request(ctx, 1) if ctx.needs_input_grad[1] and not _SKIP_PARAM_GRADS[0] else GRAD_UNWANTED      # (edges: x, weight, bias)
        if want_w != GRAD_UNWANTED:
            owner = wgrad_sink_owner(weight) if want_w == GRAD_DELIVERED else None      # (GRAD_RETURNED: see Conv3x3Fn._backward)
            if owner is None or not owner.reducer.wgrad(weight, x, x.shape[-1], cin, 0, hi, wi, kh, kw, pad, dy,
                                                        dy.shape[-1], cout, cin, 0, n, ho, wo):
                dw = torch.empty_like(weight)
                nws = _query("mnk_conv2d_wgrad_workspace_floats", n, ho, wo, cin, cout, kh, kw, pad)
                ws = SCRATCH.get("ws", nws, dy) if nws else None
                _call("mnk_conv2d_wgrad", dy, _p(x), x.shape[-1], cin, 0, hi, wi, kh, kw, pad, _p(dy), dy.shape[-1], cout,
                      _p(dw), cin, 0, n, ho, wo, _p(ws), nws)
                if owner is not None:
                    owner.add_to_sink(weight, dw)
                    dw = None
        if has_bias and ctx.needs_input_grad[2] and not _SKIP_PARAM_GRADS[0] and param_grad_request(ctx, 2) != GRAD_UNWANTED:
            db = channel_sums(dy, cout)[:cout]
        return dx, dw, db, None, None, None, None, None


class InstNormActFn(_Fn):
    """[InstanceNorm3d (affine)] -> LeakyReLU(slope) -> avg_pool (1,2,2) of the discriminator's DownBlock3D
    (modules/discriminator.py:26-33): per-frame statistics (the time axis is 1 on every call path), one fused pass."""

    @staticmethod
    def forward(ctx, y, gamma, beta, c, slope, pool, eps):
        _check_device(y)
        n, h, w, ld = y.shape
        dev = y.device
        has_norm = gamma is not None
        if has_norm:
            nws = _query("mnk_norm_workspace_floats", h * w, n, ld)
            ws = SCRATCH.get("ws", nws, y)
            sums = torch.empty(2 * n * c, dtype=torch.float32, device=dev)
            _call("mnk_norm_stats", y, _p(y), ld, h * w, n, c, _p(sums), _p(ws), nws)
            mean = torch.empty(n * c, dtype=torch.float32, device=dev)
            invstd, scale = torch.empty_like(mean), torch.empty_like(mean)
            _call("mnk_norm_finalize", y, _p(sums), float(h * w), _p(gamma), None, None, 0.0, float(eps), c, n, 0, _p(mean),
                  _p(invstd), _p(scale))
            bt = beta
        else:   # first block: no normalisation -> identity affine
            mean, invstd = _identity_affine(c, dev)          # constants, made once per (channels, device)
            scale, bt = invstd, mean
        ho, wo = (h // 2, w // 2) if pool else (h, w)
        z = torch.empty(n, ho, wo, ceil4(c), dtype=torch.float32, device=dev)
        _call("mnk_norm_act_fwd", y, _p(y), ld, _p(mean), _p(scale), _p(bt), int(has_norm), _p(z), z.shape[-1], 0, n, h, w, c,
              float(slope), int(pool))
        ctx.save_for_backward(y, mean, invstd, scale, bt)
        ctx.meta = (c, float(slope), pool, has_norm)
        return z

    @staticmethod
    def backward(ctx, dz):
        y, mean, invstd, scale, bt = ctx.saved_tensors
        c, slope, pool, has_norm = ctx.meta
        dz = dz.contiguous()
        n, h, w, ld = y.shape
        dy = torch.empty_like(y)
        dgamma = dbeta = None
        sums = None
        if has_norm:
            nws = _query("mnk_norm_workspace_floats", h * w, n, ceil4(c))
            ws = SCRATCH.get("ws", nws, y)
            sums = torch.empty(2 * n * c, dtype=torch.float32, device=y.device)
            _call("mnk_norm_act_bwd_stats", y, _p(y), ld, _p(dz), dz.shape[-1], 0, _p(mean), _p(invstd), _p(scale), _p(bt), 1,
                  n, h, w, c, slope, int(pool), _p(sums), _p(ws), nws)
            if not _SKIP_PARAM_GRADS[0]:
                per = sums.view(2, n, c).sum(dim=1)
                dbeta, dgamma = per[0], per[1]
        _call("mnk_norm_act_bwd_apply", y, _p(y), ld, _p(dz), dz.shape[-1], 0, _p(mean), _p(invstd), _p(scale), _p(bt),
              int(has_norm), _p(sums), float(h * w), int(has_norm), _p(dy), ld, n, h, w, c, slope, int(pool))
        return dy, dgamma, dbeta, None, None, None, None


_IDENTITY_AFFINE = {}


def _identity_affine(c, dev):
    t = _IDENTITY_AFFINE.get((c, dev))
    if t is None:
        t = _IDENTITY_AFFINE[(c, dev)] = (torch.zeros(c, dtype=torch.float32, device=dev),
                                          torch.ones(c, dtype=torch.float32, device=dev))
    return t


class PairL1Fn(_Fn):
    """weight * mean_batch(|generated - real|) (modules/losses.py:8-12) of one discriminator feature map, read from the
    act of the batched pass [generated | real] (2B frames) -> tensor (B,).  One launch forward, one backward; the
    feature maps never take their NCDHW form."""

    @staticmethod
    def forward(ctx, act, c, b, weight):
        _check_device(act)
        n, h, w, ld = act.shape
        assert n == 2 * b and act.is_contiguous()
        out = torch.empty(b, dtype=torch.float32, device=act.device)
        _call("mnk_pair_l1_fwd", act, _p(act), ld, h * w, c, b, float(weight), _p(out))
        ctx.save_for_backward(act)
        ctx.meta = (c, b, float(weight))
        return out

    @staticmethod
    def backward(ctx, g):
        act, = ctx.saved_tensors
        c, b, weight = ctx.meta
        n, h, w, ld = act.shape
        g = g.contiguous()
        da = torch.empty_like(act)
        _call("mnk_pair_l1_bwd", act, _p(act), ld, h * w, c, b, weight, _p(g), _p(da))
        return da, None, None, None


class PairL1TapFn(_Fn):
    """PairL1Fn as a tap on the discriminator's forward pass: (the map itself for the next block, the loss vector).  The map
    then has ONE consumer in the autograd graph, and the gradient of the next block is added inside the L1 backward kernel
    (autograd's own accumulation: one more pass over every feature map of the batched [generated | real] pass)."""

    @staticmethod
    def forward(ctx, act, c, b, weight):
        _check_device(act)
        n, h, w, ld = act.shape
        assert n == 2 * b and act.is_contiguous()
        out = torch.empty(b, dtype=torch.float32, device=act.device)
        _call("mnk_pair_l1_fwd", act, _p(act), ld, h * w, c, b, float(weight), _p(out))
        ctx.save_for_backward(act)
        ctx.meta = (c, b, float(weight))
        ctx.set_materialize_grads(False)
        return act.view_as(act), out

    @staticmethod
    def backward(ctx, g_act, g):
        if g is None:
            return g_act, None, None, None
        act, = ctx.saved_tensors
        c, b, weight = ctx.meta
        n, h, w, ld = act.shape
        if g_act is not None:
            g_act = g_act.contiguous()
        da = torch.empty_like(act)
        _call("mnk_pair_l1_bwd_add", act, _p(act), ld, h * w, c, b, weight, _p(g.contiguous()), _p(g_act), _p(da))
        return da, None, None, None


class L1MeanFn(_Fn):
    """weight * mean_batch(|prediction - target|) (modules/losses.py:8-12) of two equally shaped contiguous tensors
    (the frames themselves: reconstruction_deformed, map 0 of 'reconstruction') -> tensor (B,).  One launch each way
    instead of sub / abs / mean / mul and their four backward nodes."""

    @staticmethod
    def forward(ctx, prediction, target, weight):
        _check_device(prediction)
        assert prediction.shape == target.shape
        prediction, target = prediction.contiguous(), target.contiguous()
        b = prediction.shape[0]
        out = torch.empty(b, dtype=torch.float32, device=prediction.device)
        _call("mnk_l1_mean_fwd", prediction, _p(prediction), _p(target), prediction.numel() // b, b, float(weight), _p(out))
        ctx.save_for_backward(prediction, target)
        ctx.weight = float(weight)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if da is None and db is None:
            return None, None, None
        n = a.shape[0]
        _call("mnk_l1_mean_bwd", a, _p(a), _p(b), a.numel() // n, n, ctx.weight, _p(g.contiguous()), _p(da), _p(db))
        return da, db, None


class GanTermsFn(_Fn):
    """(generator_gan_loss, discriminator_gan_loss) of modules/losses.py:15-21 from the score maps of the batched
    discriminator pass [generated | real] (2B samples) -> two tensors (B,).  One launch each way; the score tensor is
    not sliced (a slice's backward is a zero fill and a copy)."""

    @staticmethod
    def forward(ctx, score, b, w_gen, w_disc):
        _check_device(score)
        score = score.contiguous()
        assert score.shape[0] == 2 * b
        gen = torch.empty(b, dtype=torch.float32, device=score.device)
        disc = torch.empty(b, dtype=torch.float32, device=score.device)
        _call("mnk_gan_terms_fwd", score, _p(score), score.numel() // (2 * b), b, float(w_gen), float(w_disc), _p(gen), _p(disc))
        ctx.save_for_backward(score)
        ctx.meta = (b, float(w_gen), float(w_disc))
        ctx.set_materialize_grads(False)
        return gen, disc

    @staticmethod
    def backward(ctx, ggen, gdisc):
        score, = ctx.saved_tensors
        b, w_gen, w_disc = ctx.meta
        if ggen is None and gdisc is None:
            return None, None, None, None
        ds = torch.empty_like(score)
        _call("mnk_gan_terms_bwd", score, _p(score), score.numel() // (2 * b), b, w_gen, w_disc,
              _p(ggen.contiguous()) if ggen is not None else None, _p(gdisc.contiguous()) if gdisc is not None else None, _p(ds))
        return ds, None, None, None


class LossMeansFn(_Fn):
    """[v.mean() for v in vecs] and the sum of these means (train.py:114,116) for per-sample loss vectors of one length:
    (means (n,), total ()).  One launch each way instead of stack / mean / sum and their expand / div backward passes."""

    @staticmethod
    def forward(ctx, *vecs):
        import numpy as np
        ref = vecs[0]
        _check_device(ref)
        vecs = [v.contiguous().float() for v in vecs]
        n, ln = len(vecs), vecs[0].numel()
        assert all(v.numel() == ln for v in vecs)
        out = torch.empty(n + 1, dtype=torch.float32, device=ref.device)
        ptrs = np.array([v.data_ptr() for v in vecs], dtype=np.uint64)
        _call("mnk_vec_means_fwd", ref, ptrs.ctypes.data, n, ln, _p(out))
        ctx.meta = (n, ln, [v.shape for v in vecs])
        ctx.set_materialize_grads(False)
        return out[:n], out[n]

    @staticmethod
    def backward(ctx, gmeans, gtotal):
        n, ln, shapes = ctx.meta
        if gmeans is None and gtotal is None:
            return (None,) * n
        ref = gmeans if gmeans is not None else gtotal
        gv = torch.empty(n, ln, dtype=torch.float32, device=ref.device)
        _call("mnk_vec_means_bwd", ref, _p(gmeans.contiguous()) if gmeans is not None else None,
              _p(gtotal.contiguous()) if gtotal is not None else None, n, ln, _p(gv))
        return tuple(g.view(shp) for g, shp in zip(gv.unbind(0), shapes))


class GConv1x1Fn(_Fn):
    """nn.Conv3d(kernel (1,1,1), groups=num_kp+1) of SameBlock3D (dense_motion_module.py:24-28)."""

    @staticmethod
    def forward(ctx, x, weight, bias, groups):
        _check_device(x)
        c = weight.shape[0]
        s = weight.shape[1]
        assert c == groups * s
        n, h, w, ld = x.shape
        y = torch.empty(n, h, w, ceil4(c), dtype=torch.float32, device=x.device)
        _call("mnk_gconv1x1_fwd", x, _p(x), ld, _p(weight), _p(bias), _p(y), y.shape[-1], n * h * w, groups, s)
        ctx.save_for_backward(x, weight)
        ctx.meta = (groups, s, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        groups, s, has_bias = ctx.meta
        dy = dy.contiguous()
        n, h, w, ld = x.shape
        rows = n * h * w
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _call("mnk_gconv1x1_bwd_data", dy, _p(dy), dy.shape[-1], _p(weight), _p(dx), ld, rows, groups, s)
        dw = torch.empty_like(weight)
        db = torch.empty(groups * s, dtype=torch.float32, device=x.device)
        nws = _query("mnk_gconv1x1_workspace_floats", rows, groups, s)
        ws = SCRATCH.get("ws", nws, x)
        _call("mnk_gconv1x1_bwd_weight", x, _p(x), ld, _p(dy), dy.shape[-1], _p(dw), _p(db), rows, groups, s, _p(ws), nws)
        return dx, dw, db if has_bias else None, None


class Conv1x1SigmoidFn(_Fn):
    """1x1 conv writing (B,C,D,H,W) directly: refinement_module['conv-last'] + torch.sigmoid (generator.py:48,79-80;
    act=1) or the discriminator's linear score head (discriminator.py:59,77; act=0)."""

    @staticmethod
    def forward(ctx, x, weight, bias, cin, b, act=1):
        _check_device(x)
        n, h, w, ld = x.shape
        d = n // b
        cout = weight.shape[0]
        out = torch.empty(b, cout, d, h, w, dtype=torch.float32, device=x.device)
        _call("mnk_conv1x1_fwd", x, _p(x), ld, cin, _p(weight), _p(bias), _p(out), b, d, h, w, cout, int(act))
        ctx.save_for_backward(x, weight, out)
        ctx.meta = (cin, b, d, bias is not None, int(act))
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, out = ctx.saved_tensors
        cin, b, d, has_bias, act = ctx.meta
        dout = dout.contiguous()
        n, h, w, ld = x.shape
        cout = weight.shape[0]
        need_w = ctx.needs_input_grad[1] and not _SKIP_PARAM_GRADS[0]     # (no_param_grads: input gradients only)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(weight) if need_w else None
        db = torch.empty(cout, dtype=torch.float32, device=x.device) if need_w else None
        if dx is None and dw is None:
            return None, None, None, None, None, None
        nws = _query("mnk_conv1x1_workspace_floats", n * h * w, cin, cout) if need_w else 0
        ws = SCRATCH.get("ws", nws, x) if need_w else None
        _call("mnk_conv1x1_bwd", x, _p(x), ld, cin, _p(weight), _p(out), _p(dout), _p(dx), ld, _p(dw), _p(db), b, d,
              h, w, cout, act, _p(ws), nws)
        return dx, dw, db if has_bias else None, None, None, None


# ----------------------------------------------------------------------------------------------------------------
# key-points
# ----------------------------------------------------------------------------------------------------------------
class SoftmaxKPFn(_Fn):
    """F.softmax(heatmap / T over H*W) + gaussian2kp 'matrix' (keypoint_detector.py:43-60,103-107)."""

    @staticmethod
    def forward(ctx, heat, k, temperature):
        _check_device(heat)
        n, h, w, ld = heat.shape
        dev = heat.device
        mean = torch.empty(n, k, 2, dtype=torch.float32, device=dev)
        var = torch.empty(n, k, 2, 2, dtype=torch.float32, device=dev)
        stat = torch.empty(n, k, 2, dtype=torch.float32, device=dev)
        _call("mnk_softmax_kp_fwd", heat, _p(heat), ld, n, h, w, k, float(temperature), _p(mean), _p(var), _p(stat))
        ctx.save_for_backward(heat, mean, stat)
        ctx.meta = (k, float(temperature))
        ctx.set_materialize_grads(False)     # backward makes the missing one itself (kp_variance given as a constant)
        return mean, var

    @staticmethod
    def backward(ctx, dmean, dvar):
        heat, mean, stat = ctx.saved_tensors
        k, temperature = ctx.meta
        n, h, w, ld = heat.shape
        dmean = dmean.contiguous() if dmean is not None else torch.zeros_like(mean)
        dvar = dvar.contiguous() if dvar is not None else torch.zeros(n, k, 2, 2, dtype=torch.float32, device=heat.device)
        dheat = torch.empty_like(heat)
        _call("mnk_softmax_kp_bwd", heat, _p(heat), ld, n, h, w, k, temperature, _p(mean), _p(stat), _p(dmean), _p(dvar),
              _p(dheat), ld)
        return dheat, None, None


def heatmap_argmax(heat, k):
    """(frames, K) int32: linear pixel index h * W + w of the largest heat-map logit per key point, first occurrence -- the
    integer form of the soft-argmax (keypoint_detector.py:103-104); `heat` is the key-point detector's logit act."""
    _check_device(heat)
    n, h, w, ld = heat.shape
    idx = torch.empty(n, k, dtype=torch.int32, device=heat.device)
    _call("mnk_heatmap_argmax", heat, _p(heat), ld, n, h, w, k, _p(idx))
    return idx


def kp_pixel_index(mean, size):
    """floor(size * (mean + 1) / 2) per axis, size = (W, H): the pixel the reference's Visualizer draws a key point at
    (logger.py:99-100).  mean (..., 2) fp32 -> (..., 2) int32."""
    _check_device(mean)
    m = mean.detach().contiguous().float()
    out = torch.empty(m.shape, dtype=torch.int32, device=m.device)
    _call("mnk_kp_pixel_index", m, _p(m), m.numel() // 2, int(size[0]), int(size[1]), _p(out))
    return out


# MnkVisColumn of include/monkeynet_hip.h: two pointers and five strides, 8 bytes each
VIS_COLUMN = np.dtype([("video", "<u8"), ("kp", "<u8"), ("batch_stride", "<i8"), ("chan_stride", "<i8"), ("frame_stride", "<i8"),
                       ("kp_batch_stride", "<i8"), ("kp_frame_stride", "<i8")])


def vis_grid(columns, d, kp_size, draw_border, colors, out=None):
    """The uint8 image grid of the reference's Visualizer.create_image_grid (logger.py:97-126, :151) in one launch.
    columns: up to 8 entries `video` or `(video, kp_mean)`; video (B, 3, d | 1, H, W) fp32 with contiguous H x W planes and any
    batch / channel / frame strides (one frame = the reference's `.repeat(1, 1, d, 1, 1)`, read with a frame stride of 0), kp_mean
    (B, d | 1, K, 2) fp32 with a contiguous (K, 2) tail.  colors: (K, 3) fp32 on the videos' device.
    Returns uint8 (d, B * H, ncol * W, 3)."""
    cols = [c if isinstance(c, (tuple, list)) else (c, None) for c in columns]
    first = cols[0][0]
    _check_device(first)
    b, ch, _, h, w = first.shape
    rec = np.zeros(len(cols), dtype=VIS_COLUMN)
    keep, k = [], 0
    for i, (video, kp) in enumerate(cols):
        if video.dtype != torch.float32 or video.device != first.device:
            raise ValueError("vis_grid: every video must be a float32 tensor on one device")
        if video.dim() != 5 or tuple(video.shape[:2]) != (b, ch) or tuple(video.shape[3:]) != (h, w) or video.shape[2] not in (1, d):
            raise ValueError("vis_grid: column %d has shape %s, expected (%d, %d, %d | 1, %d, %d)"
                             % (i, tuple(video.shape), b, ch, d, h, w))
        if video.stride(4) != 1 or video.stride(3) != w or min(video.stride()) < 0:
            video = video.contiguous()
        keep.append(video)
        rec[i]["video"] = video.data_ptr()
        rec[i]["batch_stride"], rec[i]["chan_stride"] = video.stride(0), video.stride(1)
        rec[i]["frame_stride"] = video.stride(2) if video.shape[2] > 1 else 0
        if kp is not None:
            if kp.dtype != torch.float32 or kp.device != first.device or kp.dim() != 4 or kp.shape[0] != b or kp.shape[3] != 2 \
                    or kp.shape[1] not in (1, d) or (k and kp.shape[2] != k):
                raise ValueError("vis_grid: key points of column %d have shape %s, expected (%d, %d | 1, K, 2) float32"
                                 % (i, tuple(kp.shape), b, d))
            k = kp.shape[2]
            if kp.stride(3) != 1 or kp.stride(2) != 2 or min(kp.stride()) < 0:
                kp = kp.contiguous()
            keep.append(kp)
            rec[i]["kp"] = kp.data_ptr()
            rec[i]["kp_batch_stride"] = kp.stride(0)
            rec[i]["kp_frame_stride"] = kp.stride(1) if kp.shape[1] > 1 else 0
    if k and (colors is None or tuple(colors.shape) != (k, 3) or colors.dtype != torch.float32 or colors.device != first.device
              or not colors.is_contiguous()):
        raise ValueError("vis_grid: colors must be a contiguous (%d, 3) float32 tensor on the videos' device" % k)
    if out is None:
        out = torch.empty(d, b * h, len(cols) * w, 3, dtype=torch.uint8, device=first.device)
    # the column table is read during the call (it travels in the kernel arguments): `rec` and `keep` only have to live until then
    _call("mnk_vis_grid", first, int(rec.ctypes.data), len(cols), b, ch, d, h, w, k, float(kp_size), int(bool(draw_border)),
          _p(colors) if k else None, _p(out))
    return out


def frames_to_strip(video, out=None):
    """(C = 3, D, H, W) fp32 -> uint8 (H, D * W, 3): the frame strip the evaluation loops save as .png
    (reconstruction.py:66-68, prediction.py:137-139)."""
    _check_device(video)
    if video.dim() != 4 or video.dtype != torch.float32:
        raise ValueError("frames_to_strip: expected a (3, D, H, W) float32 tensor, got %s %s" % (tuple(video.shape), video.dtype))
    c, d, h, w = video.shape
    if video.stride(3) != 1 or video.stride(2) != w or min(video.stride()) < 0:
        video = video.contiguous()
    if out is None:
        out = torch.empty(h, d * w, 3, dtype=torch.uint8, device=video.device)
    _call("mnk_frames_to_strip", video, _p(video), c, video.stride(0), video.stride(1), d, h, w, _p(out))
    return out


class ClipVarianceFn(_Fn):
    """var * max(clip, sigma_min(var)) / sigma_min(var) on (..., 2, 2) covariances (keypoint_detector.py:62-65,
    modules/util.py:244-255) in one kernel instead of ~25 element-wise launches (+ ~60 in the backward)."""

    @staticmethod
    def forward(ctx, var, clip, mode="stable"):
        """mode: "stable" (default; sigma_min = |det| / sigma_max) | "reference" (the reference's own fp32 closed form
        sqrt((s1 - s2) / 2), modules/util.py:244-255 -- for parity work; it returns NaN on nearly singular covariances)"""
        _check_device(var)
        if mode not in ("stable", "reference"):
            raise ValueError("clip_variance_mode must be 'stable' or 'reference', got %r" % (mode,))
        var = var.contiguous().float()
        out = torch.empty_like(var)
        ctx.ref_mode = int(mode == "reference")
        _call("mnk_kp_clip_variance_fwd", var, _p(var), float(clip), var.numel() // 4, _p(out), ctx.ref_mode)
        ctx.save_for_backward(var)
        ctx.clip = float(clip)
        return out

    @staticmethod
    def backward(ctx, dout):
        var, = ctx.saved_tensors
        dout = dout.contiguous()
        dvar = torch.empty_like(var)
        _call("mnk_kp_clip_variance_bwd", var, _p(var), ctx.clip, var.numel() // 4, _p(dout), _p(dvar), ctx.ref_mode)
        return dvar, None, None


class MovementEmbeddingFn(_Fn):
    """MovementEmbeddingModule.forward (movement_embedding.py:42-92) -> act with kp-major channel order."""

    @staticmethod
    def forward(ctx, img, mean_d, var_d, mean_s, var_s, cfg):
        (b, d, h, w, k, cimg, add_bg, use_heatmap, use_difference, use_deformed, heatmap_diff, norm_const,
         const_var) = cfg
        ref = mean_d
        _check_device(ref)
        dev = ref.device
        mean_d = mean_d.contiguous().float()
        mean_s = mean_s.contiguous().float()
        var_d = var_d.contiguous().float() if var_d is not None else None
        var_s = var_s.contiguous().float() if var_s is not None else None
        slots = k + int(add_bg)
        per = int(use_heatmap) + 2 * int(use_difference) + (cimg if use_deformed else 0)
        ld_out = ceil4(slots * per)
        norm_d = norm_s = None
        norm_c = float(norm_const) if norm_const != "sum" else 0.0
        if norm_const == "sum" and use_heatmap:
            norm_d = torch.empty(b * d * k, dtype=torch.float32, device=dev)
            norm_s = torch.empty(b * k, dtype=torch.float32, device=dev)
            _call("mnk_gaussian_sums", ref, _p(mean_d), _p(var_d), const_var, b * d * k, h, w, _p(norm_d))
            _call("mnk_gaussian_sums", ref, _p(mean_s), _p(var_s), const_var, b * k, h, w, _p(norm_s))
        out = torch.empty(b * d, h, w, ld_out, dtype=torch.float32, device=dev)
        args = (_p(img), img.shape[-1] if img is not None else 0, cimg, _p(mean_d), _p(var_d), _p(mean_s), _p(var_s),
                float(const_var), b, d, h, w, k, int(add_bg), int(use_heatmap), int(use_difference), int(use_deformed),
                int(heatmap_diff), norm_c, _p(norm_d), _p(norm_s))
        _call("mnk_movement_embedding_fwd", ref, *args, _p(out), ld_out)
        ctx.save_for_backward(img, mean_d, var_d, mean_s, var_s, norm_d, norm_s)
        ctx.cfg = cfg
        ctx.norm_c = norm_c
        return out

    @staticmethod
    def backward(ctx, dout):
        img, mean_d, var_d, mean_s, var_s, norm_d, norm_s = ctx.saved_tensors
        (b, d, h, w, k, cimg, add_bg, use_heatmap, use_difference, use_deformed, heatmap_diff, norm_const,
         const_var) = ctx.cfg
        dout = dout.contiguous()
        dev = dout.device
        gmd = torch.empty(b * d, k, 2, dtype=torch.float32, device=dev)
        gms = torch.empty(b * d, k, 2, dtype=torch.float32, device=dev)
        gvd = gvs = None
        if var_d is not None:
            gvd = torch.empty(b * d, k, 4, dtype=torch.float32, device=dev)
            gvs = torch.empty(b * d, k, 4, dtype=torch.float32, device=dev)
        args = (_p(img), img.shape[-1] if img is not None else 0, cimg, _p(mean_d), _p(var_d), _p(mean_s), _p(var_s),
                float(const_var), b, d, h, w, k, int(add_bg), int(use_heatmap), int(use_difference), int(use_deformed),
                int(heatmap_diff), ctx.norm_c, _p(norm_d), _p(norm_s))
        _call("mnk_movement_embedding_bwd", dout, *args, _p(dout), dout.shape[-1], _p(gmd), _p(gvd), _p(gms), _p(gvs))
        g_mean_d = gmd.view(b, d, k, 2)
        g_mean_s = gms.view(b, d, k, 2).sum(dim=1, keepdim=True) if d > 1 else gms.view(b, 1, k, 2)
        g_var_d = g_var_s = None
        if gvd is not None:
            g_var_d = gvd.view(b, d, k, 2, 2)
            g_var_s = gvs.view(b, d, k, 2, 2).sum(dim=1, keepdim=True) if d > 1 else gvs.view(b, 1, k, 2, 2)
            if not use_heatmap:
                g_var_d = g_var_s = None
        g_img = None
        if img is not None and use_deformed and ctx.needs_input_grad[0]:
            # (no caller of the reference asks for it -- source images are data: a launch of its own, only when somebody does)
            g_img = torch.empty_like(img)
            _call("mnk_movement_embedding_img_bwd", dout, img.shape[-1], cimg, _p(mean_d), _p(mean_s), b, d, h, w, k, int(add_bg),
                  int(use_heatmap), int(use_difference), _p(dout), dout.shape[-1], _p(g_img))
        return g_img, g_mean_d, g_var_d, g_mean_s, g_var_s, None


class MotionFieldKPFn(_Fn):
    """MotionFieldFn's mask form with kp_source.mean - kp_driving.mean formed inside the kernels (one driving frame per
    video): no subtraction / concatenation / zero-slot launches, and the two key-point gradients come out of the backward
    kernel.  mean_s, mean_d: (B,1,K,2)."""

    @staticmethod
    def forward(ctx, pred, mean_s, mean_d, k, use_corr):
        _check_device(pred)
        n, h, w, ld = pred.shape
        ms, md = mean_s.contiguous().float(), mean_d.contiguous().float()
        assert ms.numel() == n * k * 2 and md.numel() == n * k * 2
        field = torch.empty(n, h, w, 2, dtype=torch.float32, device=pred.device)
        _call("mnk_motion_field_kp_fwd", pred, _p(pred), ld, _p(ms), _p(md), n, h, w, k, int(use_corr), _p(field))
        ctx.save_for_backward(pred, ms, md)
        ctx.meta = (k, use_corr, mean_s.shape)
        return field

    @staticmethod
    def backward(ctx, dfield):
        pred, ms, md = ctx.saved_tensors
        k, use_corr, shape = ctx.meta
        n, h, w, ld = pred.shape
        dfield = dfield.contiguous()
        dpred = torch.empty_like(pred)
        g = torch.empty(2, *shape, dtype=torch.float32, device=pred.device)
        _call("mnk_motion_field_kp_bwd", pred, _p(pred), ld, _p(ms), _p(md), _p(dfield), n, h, w, k, int(use_corr), _p(dpred),
              ld, _p(g[0]), _p(g[1]))
        return dpred, g[0], g[1], None, None


class MotionFieldFn(_Fn):
    """mask softmax, sum_k m_k * delta_k + correction + identity grid (dense_motion_module.py:52-73) -> (N,h,w,2)."""

    @staticmethod
    def forward(ctx, pred, delta, k, use_mask, use_corr):
        _check_device(pred)
        n, h, w, ld = pred.shape
        delta = delta.contiguous().float() if delta is not None else None
        field = torch.empty(n, h, w, 2, dtype=torch.float32, device=pred.device)
        _call("mnk_motion_field_fwd", pred, _p(pred), ld, _p(delta), n, h, w, k, int(use_mask), int(use_corr), _p(field))
        ctx.save_for_backward(pred, delta)
        ctx.meta = (k, use_mask, use_corr)
        return field

    @staticmethod
    def backward(ctx, dfield):
        pred, delta = ctx.saved_tensors
        k, use_mask, use_corr = ctx.meta
        n, h, w, ld = pred.shape
        dfield = dfield.contiguous()
        dpred = torch.empty_like(pred)
        ddelta = torch.empty(n, k + 1, 2, dtype=torch.float32, device=pred.device)
        _call("mnk_motion_field_bwd", pred, _p(pred), ld, _p(delta), _p(dfield), n, h, w, k, int(use_mask), int(use_corr),
              _p(dpred), ld, _p(ddelta))
        return dpred, (ddelta if delta is not None else None), None, None, None


def _warp_frames(field, inp):
    """driving frames per source image: the field has rows v*frames + f, the source one image per video (generator.py:51-58
    repeats the source along the depth axis instead)"""
    n, m = field.shape[0], inp.shape[0]
    if m <= 0 or n % m:
        raise ValueError("warp: %d field rows cannot share %d source images" % (n, m))
    return n // m


def _deform_fwd(inp, ld_in, c, h, w, field, hf, wf, mode, out, n, frames):
    if frames == 1:
        _call("mnk_deform_fwd", inp, _p(inp), ld_in, c, h, w, _p(field), hf, wf, mode, _p(out), out.shape[-1], 0, n)
    else:
        _call("mnk_deform_shared_fwd", inp, _p(inp), ld_in, c, h, w, _p(field), hf, wf, mode, _p(out), out.shape[-1], 0, n,
              frames)


def _deform_bwd(inp, ld_in, c, h, w, field, hf, wf, mode, dout, dinp, dfield, n, frames):
    nws = _query("mnk_deform_bwd_workspace_floats", c, h, w, n)         # (n: the field's rows, whatever the source has)
    if frames == 1:
        _call("mnk_deform_bwd", inp, _p(inp), ld_in, c, h, w, _p(field), hf, wf, mode, _p(dout), dout.shape[-1], 0,
              _p(dinp), _p(dfield), n, _p(SCRATCH.get("ws", nws, inp)), nws)
    else:
        _call("mnk_deform_shared_bwd", inp, _p(inp), ld_in, c, h, w, _p(field), hf, wf, mode, _p(dout), dout.shape[-1], 0,
              _p(dinp), _p(dfield), n, frames, _p(SCRATCH.get("ws", nws, inp)), nws)


class WarpSkipFn(_Fn):
    """deform_input (generator.py:51-58) of one skip tensor, with the nearest-resized key-point embedding written
    behind it in the same buffer (generator.py:72-73): out = [warp(inp, field) | resize(emb)].  A source with fewer rows than
    the field is shared by the frames of its video (_warp_frames): out has the field's rows, d input the source's shape."""

    @staticmethod
    def forward(ctx, inp, field, emb, c, ke, mode):
        _check_device(inp)
        _, h, w, ld_in = inp.shape
        n, hf, wf, _ = field.shape
        frames = _warp_frames(field, inp)
        # c a multiple of 4: the warp writes whole channel quads and the resized embedding, copied with its (zero) pad
        # channels, the rest of every pixel row -- no zero fill of the output
        whole = c % 4 == 0 and (emb is None or emb.shape[-1] == ceil4(ke))
        out = (torch.empty if whole else torch.zeros)(n, h, w, ceil4(c + ke), dtype=torch.float32, device=inp.device)
        _deform_fwd(inp, ld_in, c, h, w, field, hf, wf, mode, out, n, frames)
        if emb is not None:
            _call("mnk_resize_nearest" if mode == 0 else "mnk_resize_bilinear", inp, _p(emb), emb.shape[-1], emb.shape[1], emb.shape[2], _p(out), out.shape[-1], c,
                  h, w, n, ceil4(ke) if whole else ke)
        ctx.save_for_backward(inp, field, emb)
        ctx.meta = (c, ke, mode)
        return out

    @staticmethod
    def backward(ctx, dout):
        inp, field, emb = ctx.saved_tensors
        c, ke, mode = ctx.meta
        dout = dout.contiguous()
        _, h, w, ld_in = inp.shape
        n, hf, wf, _ = field.shape
        dinp = torch.empty_like(inp) if ctx.needs_input_grad[0] else None       # written by the gather pass
        dfield = torch.zeros_like(field) if ctx.needs_input_grad[1] else None    # added to
        if dinp is not None or dfield is not None:
            _deform_bwd(inp, ld_in, c, h, w, field, hf, wf, mode, dout, dinp, dfield, n, _warp_frames(field, inp))
        demb = None
        if emb is not None and ctx.needs_input_grad[2]:
            # nearest: the adjoint is a gather that writes every source pixel; with c a multiple of 4 it also reads the
            # (zero) pad channels of dout and so writes demb's pads itself
            whole = mode == 0 and c % 4 == 0 and emb.shape[-1] == ceil4(ke) and dout.shape[-1] == c + emb.shape[-1]
            demb = torch.empty_like(emb) if whole else torch.zeros_like(emb)
            _call("mnk_resize_nearest_bwd" if mode == 0 else "mnk_resize_bilinear_bwd", inp, _p(dout), dout.shape[-1], c, h, w, _p(demb), emb.shape[-1], emb.shape[1],
                  emb.shape[2], n, emb.shape[-1] if whole else ke)
        return dinp, dfield, demb, None, None, None


WARP_LEVEL = np.dtype([("inp", "<u8"), ("out", "<u8"), ("dout", "<u8"), ("dinp", "<u8"), ("ld_in", "<i4"), ("C", "<i4"),
                       ("h", "<i4"), ("w", "<i4"), ("ld_out", "<i4"), ("ke", "<i4"), ("emb_off", "<i4"), ("reserved", "<i4")])


class WarpAllFn(_Fn):
    """Every deform_input of one generator forward (generator.py:66-73 the skips, :78 the source frame) as ONE autograd node.
    They all read the same deformation field, so as separate nodes each backward zero-fills its own field gradient and
    autograd adds the eight of them up; here one gather per field texel sums the levels in order (mnk_warp_levels_bwd:
    deterministic, nothing is zero-filled).  forward(field, emb, mode, specs, *inps) with specs = ((c, ke), ...) per input; returns one
    [warp(inp) | resize(emb)] act per input (ke = 0: no embedding behind it)."""

    @staticmethod
    def forward(ctx, field, emb, mode, specs, *inps):
        _check_device(field)
        n, hf, wf, _ = field.shape
        frames = _warp_frames(field, inps[0])
        if any(inp.shape[0] != inps[0].shape[0] for inp in inps):
            raise ValueError("warp: the levels differ in their number of source images")
        outs = []
        ctx.multi = len(inps) <= 12 and knobs.form("WARP_LEVELS")
        if ctx.multi:         # one launch for the warps and embedding copies of all levels (mnk_warp_levels_fwd)
            lv = np.zeros(len(inps), dtype=WARP_LEVEL)
            for i, (inp, (c, ke)) in enumerate(zip(inps, specs)):
                _, h, w, ld_in = inp.shape
                e = emb if ke else None
                # (the launch writes every channel of every row -- warp, embedding, pad channels: no zero fill)
                out = torch.empty(n, h, w, ceil4(c + ke), dtype=torch.float32, device=inp.device)
                lv[i] = (inp.data_ptr(), out.data_ptr(), 0, 0, ld_in, c, h, w, out.shape[-1], ke if e is not None else 0, c, 0)
                outs.append(out)
            tail = (n,) if frames == 1 else (n, frames)
            _call("mnk_warp_levels_fwd" if frames == 1 else "mnk_warp_levels_shared_fwd", field, lv.ctypes.data, len(inps),
                  _p(field), hf, wf, mode, _p(emb), emb.shape[-1] if emb is not None else 0,
                  emb.shape[1] if emb is not None else 0, emb.shape[2] if emb is not None else 0, *tail)
            ctx.save_for_backward(field, emb, *inps)
            ctx.meta = (mode, tuple(specs))
            ctx.set_materialize_grads(False)
            return tuple(outs)
        for inp, (c, ke) in zip(inps, specs):
            _, h, w, ld_in = inp.shape
            e = emb if ke else None
            whole = c % 4 == 0 and (e is None or e.shape[-1] == ceil4(ke))      # see WarpSkipFn.forward
            out = (torch.empty if whole else torch.zeros)(n, h, w, ceil4(c + ke), dtype=torch.float32, device=inp.device)
            _deform_fwd(inp, ld_in, c, h, w, field, hf, wf, mode, out, n, frames)
            if e is not None:
                _call("mnk_resize_nearest" if mode == 0 else "mnk_resize_bilinear", inp, _p(e), e.shape[-1], e.shape[1],
                      e.shape[2], _p(out), out.shape[-1], c, h, w, n, ceil4(ke) if whole else ke)
            outs.append(out)
        ctx.save_for_backward(field, emb, *inps)
        ctx.meta = (mode, tuple(specs))
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        field, emb = ctx.saved_tensors[:2]
        inps = ctx.saved_tensors[2:]
        mode, specs = ctx.meta
        nrows, hf, wf, _ = field.shape
        frames = _warp_frames(field, inps[0])
        # the gradients of all warps (d input of every level, d field) are slices of ONE buffer.  The acts come first (their
        # sizes are multiples of 4 floats: every slice stays 16-byte aligned for the float4 readers downstream), the field
        # last.  The one-launch form writes every element; the per-level form adds the levels' field gradients up.
        want_field = ctx.needs_input_grad[0] and any(d is not None for d in douts)
        want = [ctx.needs_input_grad[4 + i] and douts[i] is not None for i in range(len(inps))]
        sizes = [inp.numel() if wnt else 0 for inp, wnt in zip(inps, want)] + [field.numel() if want_field else 0]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=field.device) if sum(sizes) else None
        offs = [sum(sizes[:k]) for k in range(len(sizes))]
        dfield = flat[offs[-1]:offs[-1] + sizes[-1]].view_as(field) if want_field else None
        demb = None
        dinps = []
        if ctx.multi and any(d is not None for d in douts):
            live = [i for i, d in enumerate(douts) if d is not None]        # (a level whose output went nowhere: no gradient)
            lv = np.zeros(len(live), dtype=WARP_LEVEL)
            keep = []
            want_emb = emb is not None and ctx.needs_input_grad[1] and any(specs[i][1] for i in live)
            dinps = [None] * len(inps)
            for j, i in enumerate(live):
                inp, (c, ke) = inps[i], specs[i]
                dout = douts[i].contiguous()
                keep.append(dout)
                _, h, w, ld_in = inp.shape
                dinps[i] = flat[offs[i]:offs[i] + sizes[i]].view_as(inp) if want[i] else None
                lv[j] = (inp.data_ptr(), 0, dout.data_ptr(), dinps[i].data_ptr() if dinps[i] is not None else 0, ld_in, c, h, w,
                         dout.shape[-1], ke if want_emb else 0, c, 0)
            if want_emb:
                demb = torch.empty_like(emb)
            nws = _query("mnk_warp_levels_bwd_workspace_floats", lv.ctypes.data, len(live), nrows)    # (the field's rows)
            tail = (nrows,) if frames == 1 else (nrows, frames)
            _call("mnk_warp_levels_bwd" if frames == 1 else "mnk_warp_levels_shared_bwd", field, lv.ctypes.data, len(live),
                  _p(field), hf, wf, mode, _p(dfield), _p(demb), emb.shape[-1] if emb is not None else 0,
                  emb.shape[1] if emb is not None else 0, emb.shape[2] if emb is not None else 0, *tail,
                  _p(SCRATCH.get("ws", nws, field)), nws)
            return (dfield, demb, None, None) + tuple(dinps)
        if dfield is not None:
            dfield.zero_()
        for i, (inp, (c, ke), dout) in enumerate(zip(inps, specs, douts)):
            if dout is None:
                dinps.append(None)
                continue
            dout = dout.contiguous()
            _, h, w, ld_in = inp.shape
            n = nrows
            dinp = flat[offs[i]:offs[i] + sizes[i]].view_as(inp) if want[i] else None
            if dinp is not None or dfield is not None:
                _deform_bwd(inp, ld_in, c, h, w, field, hf, wf, mode, dout, dinp, dfield, n, frames)
            dinps.append(dinp)
            if ke and emb is not None and ctx.needs_input_grad[1]:
                # the first contribution writes demb (nearest: a gather over the source pixels that, with c a multiple of 4,
                # also copies the zero pad channels of dout), the others are added by the kernels
                whole = mode == 0 and c % 4 == 0 and emb.shape[-1] == ceil4(ke) and dout.shape[-1] == c + emb.shape[-1]
                first = demb is None
                if first:
                    demb = torch.empty_like(emb) if whole else torch.zeros_like(emb)
                name = ("mnk_resize_nearest_bwd" if first else "mnk_resize_nearest_bwd_accumulate") if mode == 0 \
                    else "mnk_resize_bilinear_bwd"                  # (bilinear: added to the zeroed buffer by a gather)
                _call(name, inp, _p(dout), dout.shape[-1], c, h, w, _p(demb), emb.shape[-1], emb.shape[1], emb.shape[2], n,
                      emb.shape[-1] if whole else ke)
        return (dfield, demb, None, None) + tuple(dinps)


# convenience wrappers ---------------------------------------------------------------------------------------------
def to_act(x5, step=1):
    if isinstance(x5, U8Frames):
        return u8_to_act(x5, int(step))
    if isinstance(x5, StackedBatch):
        return ToActPairFn.apply(x5.parts[0], x5.parts[1], step)
    return ToActFn.apply(x5, int(step))


def from_act(a, c, b):
    return FromActFn.apply(a, c, b)


def step_from_scale(scale_factor):
    if scale_factor == 1:
        return 1
    step = int(round(1.0 / scale_factor))
    if abs(step * scale_factor - 1.0) > 1e-6:
        raise NotImplementedError("only scale factors 1/integer are used by the reference configs; got %r" % scale_factor)
    return step
