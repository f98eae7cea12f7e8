"""Animation sessions: one source image, a driving stream that is long or arrives over time (demo.py:60-71, transfer.py:65-79).

Two things outlive a call here that mnk.engine.Transfer computes per call:

* the encoded source -- MotionTransferGenerator.encode_source: the appearance encoder's skip acts and the source's layout
  conversions, computed once per set_source();
* the anchor of the key-point normalisation -- transfer.py:31-62 moves and rescales every frame relative to frame 0 of the WHOLE
  driving video (its mean, its covariance, the convex-hull area of [0, 0]).  KpAnchor keeps those of the first frame pushed, on the
  device, behind a device-side flag: mnk_kp_anchor_update fills them when the flag is clear and is a no-op afterwards, so the push
  that anchors and every later push issue the same launches and one captured program serves both.
"""
import torch

from . import _lib
from . import graphs as mgraphs
from . import ops as mops


class KpAnchor:
    """The first driving frame's key-points of a stream, kept on the device: mean [B][K][2], var [B][K][4] (key-points with a
    covariance), the hull area of batch entry 0 (the reference's `[0, 0]`, transfer.py:34-36) and the int32 flag `anchored`.
    mnk.engine.normalize_kp(..., anchor=a) anchors on the first call after a reset and normalises against the anchor from then
    on.  source_area: optionally the hull area of the source's key-points [0, 0] as a device scalar, computed once by the owner
    (None: normalize_kp computes it per call)."""

    def __init__(self):
        self.mean = self.var = self.area = self.flag = None
        self.source_area = None

    def prepare(self, b, k, has_var, device):
        """allocate for (B, K) key-points (cleared), or check that the buffers fit them"""
        if self.flag is None:
            self.mean = torch.zeros(b, k, 2, dtype=torch.float32, device=device)
            self.var = torch.zeros(b, k, 4, dtype=torch.float32, device=device) if has_var else None
            self.area = torch.zeros(1, dtype=torch.float32, device=device)
            self.flag = torch.zeros(1, dtype=torch.int32, device=device)
            return
        if tuple(self.mean.shape) != (b, k, 2) or (self.var is not None) != bool(has_var) or self.mean.device != torch.device(device):
            raise ValueError("the anchor holds key-points of shape (B, K) = %s %s a covariance on %s; got (%d, %d) %s one on %s"
                             % (tuple(self.mean.shape[:2]), "with" if self.var is not None else "without", self.mean.device, b, k,
                                "with" if has_var else "without", device))

    def reset(self):
        """forget the anchor: the next normalisation anchors again"""
        if self.flag is not None:
            self.flag.zero_()

    @property
    def anchored(self):
        """whether an anchor is held (reads the device flag: a host synchronisation)"""
        return self.flag is not None and bool(int(self.flag.cpu()[0]))

    def snapshot(self):
        if self.flag is None:
            return None
        return [None if t is None else t.clone() for t in (self.mean, self.var, self.area, self.flag)]

    def restore(self, snap):
        if snap is None:
            return self.reset()
        for t, c in zip((self.mean, self.var, self.area, self.flag), snap):
            if t is not None:
                t.copy_(c)


def _cat_kp(parts):
    return {k: torch.cat([p[k] for p in parts], dim=1) for k in parts[0]}


class AnimationSession:
    """One source, many driving frames, pushed in chunks:

        s = AnimationSession(kp_detector, generator, normalization_params)
        s.set_source(source_image)          # (B, C, 1, H, W)
        out = s.push(frames)                # (B, C, n, H, W), n >= 1

    push returns the dict mnk.engine.Transfer returns for those n frames -- video_prediction / video_deformed (B, C, n, H, W),
    kp_driving, kp_source, kp_norm -- and equals what Transfer(shared_source=True) gives for the same frames inside the whole video:
    the key-points are normalised against the FIRST frame pushed since set_source() / reset(), not against the chunk's own.  A push
    is one detector call on the n frames, mnk_kp_anchor_update, mnk_kp_normalize_anchored and one generator call on the cached
    source state (no appearance encoder, no source conversion).

    normalization_params: transfer.py's dict (movement_mult, move_location, adapt_variance, clip_mean).  None, or neither
    move_location nor adapt_variance: the key-points pass through unchanged and no anchor is kept -- reconstruction.py:12-25's
    `generate`.  clip_mean without move_location raises the reference's NameError at push().
    movement_mult scales by the convex-hull areas of batch entry 0 only (`[0, 0]`), as the reference does.

    set_source(): key-points of the source, their hull area, generator.encode_source; clears the anchor.  Called again with the
    same shapes it writes the cached tensors in place, so captured programs stay valid.  The cached state holds activations: after
    load_state_dict (or any other change of the weights) call set_source again.
    reset(): forget the anchor (the next push anchors again); the source stays.
    frames_pushed: frames pushed since set_source() / reset().

    use_graph: None -- captured on a device build (the emulator always runs eager).  One linear hipGraph per (B, n) push shape;
    the program of an anchoring push and of a later one is the same.  The tensors a captured push returns are static buffers that
    the next push of that shape overwrites: clone what must survive.  A program is captured with frozen weights, like
    mnk.dropin.EvalRunner's (a push of a few frames would otherwise spend most of its launches re-packing weights): it reads the
    packed weights and the evaluation-mode norm coefficients of the moment of capture, and is captured again when a parameter, a
    buffer or the optimiser epoch changed -- the cached source is not re-encoded by that: set_source() does it.
    precision / fuse_norm / skinny: one ops.EvalOptions value, as in Reconstructor / Transfer; a captured program keeps the
    options it was built with.

    uint8 frames: set_source and push also take an ops.U8Frames or a bare 5-d torch.uint8 tensor, which is taken as channel-last
    frames (B, n, H, W, C), C = 1 / 3 / 4 -- what a decoder or a camera hands over (frames_dataset.py:14-40).  The bytes go straight
    into the kernels' layout (mnk_u8_to_nhwc); they may live on the host, pinned or not: the push copies them to the device once, a
    quarter of the fp32 bytes, and a captured program's static input is that uint8 buffer.
    output="uint8": video_prediction / video_deformed come back as uint8 (B, n, H, W, C), `(255 * out).astype(np.uint8)`
    channel-last (demo.py:69-71), written by the generator's last kernels; the fp32 tensors are not made.  Programs are keyed by
    (B, n) and, where they are not float / float, by the input kind and the output kind."""

    def __init__(self, kp_detector, generator, normalization_params=None, use_graph=None, precision="fp32", fuse_norm=False,
                 skinny=False, output="float"):
        self.output = mops.check_output(output)
        self.kp_detector, self.generator = kp_detector.eval(), generator.eval()
        self.options = mops.EvalOptions(mops.check_precision(precision), bool(fuse_norm), bool(skinny))
        self.precision, self.fuse_norm, self.skinny = self.options
        self.params = dict(normalization_params) if normalization_params is not None else None
        self.use_graph = use_graph
        self.anchor = KpAnchor()
        self.frames_pushed = 0
        self._source = self._kp_source = self._state = None
        self._programs = {}
        self._weights = ()
        self._cap = None

    # ---- state -----------------------------------------------------------------------------------------------------------------
    def _flag(self, name):
        return bool(self.params.get(name, False)) if self.params is not None else False

    def _normalizes(self):
        """whether normalize_kp would do anything: transfer.py:44-60 with neither option returns the key-points as they are"""
        has_var = self._kp_source is not None and 'var' in self._kp_source
        return self._flag("move_location") or (self._flag("adapt_variance") and has_var)

    def _graph_on(self):
        dev = self._source.device
        on_device = _lib.lib().is_device_build and dev.type == "cuda"
        return on_device if self.use_graph is None else (bool(self.use_graph) and on_device)

    def set_source(self, source_image):
        source_image = mops.as_frames(source_image, mops.module_device(self.generator))
        if source_image.dim() != 5 or source_image.shape[2] != 1:
            raise ValueError("set_source takes (B, C, 1, H, W); got %s" % (tuple(source_image.shape),))
        self._weights = [t for m in (self.kp_detector, self.generator) for t in list(m.parameters()) + list(m.buffers())]
        with torch.no_grad(), mops.eval_options(*self.options):
            kp_source = self.kp_detector(source_image)
            state = self.generator.encode_source(source_image)
            area = None
            if self._flag("movement_mult") and (self._flag("move_location") or (self._flag("adapt_variance") and 'var' in kp_source)):
                mean = kp_source['mean'].contiguous().float()
                area = torch.empty(1, dtype=torch.float32, device=mean.device)
                mops._call("mnk_kp_hull_area", mean, mops._p(mean), mean.shape[2], mops._p(area))    # kp_source['mean'][0, 0]
            same = (self._source is not None and self._source.shape == source_image.shape
                    and mops.frame_kind(self._source) == mops.frame_kind(source_image)
                    and self._source.device == source_image.device and set(self._kp_source) == set(kp_source))
            if same:
                self._source.copy_(source_image)
                for k, v in kp_source.items():
                    self._kp_source[k].copy_(v)
                self._state.copy_from(state)
                if area is not None:
                    self.anchor.source_area.copy_(area)
            else:
                self._programs.clear()
                self._source = source_image.clone() if mops.is_u8(source_image) else source_image.detach().float().clone()
                self._kp_source = {k: v.clone() for k, v in kp_source.items()}
                self._state = state
                self.anchor = KpAnchor()
                self.anchor.source_area = area
                b, _, k, _ = kp_source['mean'].shape
                self.anchor.prepare(b, k, 'var' in kp_source, source_image.device)
        self.reset()

    def reset(self):
        self.anchor.reset()
        self.frames_pushed = 0

    # ---- push ------------------------------------------------------------------------------------------------------------------
    def _forward(self, frames):
        from . import engine
        kp_driving = self.kp_detector(frames)                            # (B, n, K, .)
        if self._normalizes():
            kp_norm = engine.normalize_kp(kp_driving, self._kp_source, anchor=self.anchor, **self.params)
        else:
            kp_norm = {k: v for k, v in kp_driving.items()}
        out = self.generator(self._source, kp_driving=kp_norm, kp_source=self._kp_source, source_state=self._state,
                             output=self.output)
        return {"video_prediction": out["video_prediction"], "video_deformed": out["video_deformed"],
                "kp_driving": kp_driving, "kp_source": self._kp_source, "kp_norm": kp_norm}

    def _capture(self, frames, fp):
        """one linear hipGraph for this push shape, with frozen weights.  The warm-up pushes run the real launches, the anchoring
        one included: the anchor and its flag are put back afterwards, so the program starts from the state the session was in.
        Every program of the session warms up and is captured on one stream: the packed-weight and norm-coefficient caches the
        capture reads are keyed by it."""
        # (uint8 frames stay bytes: the static input is the uint8 buffer, on the device wherever the caller's frames live)
        static_in = frames.to(self._source.device).clone() if mops.is_u8(frames) else frames.detach().float().clone()
        snap = self.anchor.snapshot()
        if self._cap is None:
            self._cap = torch.cuda.Stream()
        mgraphs.warm_up(lambda: self._forward(static_in), 2, stream=self._cap)
        graph, static_out = mgraphs.capture(lambda: self._forward(static_in), stream=self._cap, frozen=True)
        self.anchor.restore(snap)
        return graph, static_in, static_out, fp, mops.held_eval_coeffs((self.kp_detector, self.generator))

    def push(self, frames):
        if self._state is None:
            raise ValueError("push() before set_source()")
        frames = mops.as_frames(frames)
        if frames.dim() != 5 or frames.shape[2] < 1:
            raise ValueError("push takes (B, C, n, H, W) with n >= 1; got %s" % (tuple(frames.shape),))
        b, c, n, h, w = frames.shape
        if (b, c, h, w) != (self._source.shape[0], self._source.shape[1]) + tuple(self._source.shape[3:]):
            raise ValueError("the frames' (B, C, H, W) = %s differ from the source's %s"
                             % ((b, c, h, w), (self._source.shape[0], self._source.shape[1]) + tuple(self._source.shape[3:])))
        if self._flag("clip_mean") and not self._flag("move_location"):
            raise NameError("clip_mean without move_location is an error in the reference too (transfer.py:49)")
        with torch.no_grad(), mops.eval_options(*self.options):
            if self._graph_on():
                # (B, n) for float frames in and out, as ever; other input / output kinds append theirs: (B, n, kind, output)
                kinds = (mops.frame_kind(frames), self.output)
                key = (b, n) if kinds == (("float", c), "float") else (b, n) + kinds
                prog, fp = self._programs.get(key), mops.weights_fingerprint(self._weights)
                if prog is None or prog[3] != fp:
                    prog = self._programs[key] = self._capture(frames, fp)
                graph, static_in, out = prog[:3]
                static_in.copy_(frames, non_blocking=True)
                graph.replay()
            else:
                out = self._forward(frames.to(self._source.device) if mops.is_u8(frames) else frames)
        self.frames_pushed += n
        return out

    def animate(self, driving_video, chunk):
        """the whole of `driving_video` (B, C, d, H, W) in pushes of `chunk` frames from a fresh anchor, results concatenated: what
        Transfer(shared_source=True) returns for it, with the activations of one chunk alive at a time"""
        self.reset()
        parts = []
        driving_video = mops.as_frames(driving_video)
        for i in range(0, driving_video.shape[2], chunk):
            out = self.push(driving_video[:, :, i:i + chunk])
            parts.append({k: (v.clone() if torch.is_tensor(v) else {kk: t.clone() for kk, t in v.items()}) for k, v in out.items()}
                         if self._graph_on() else out)
        fdim = 1 if self.output == "uint8" else 2            # the frame axis of (B, n, H, W, C) / (B, C, n, H, W)
        return {"video_prediction": torch.cat([p["video_prediction"] for p in parts], dim=fdim),
                "video_deformed": torch.cat([p["video_deformed"] for p in parts], dim=fdim),
                "kp_driving": _cat_kp([p["kp_driving"] for p in parts]), "kp_source": parts[0]["kp_source"],
                "kp_norm": _cat_kp([p["kp_norm"] for p in parts])}
