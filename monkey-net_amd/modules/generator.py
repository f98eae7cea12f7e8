"""MotionTransferGenerator (modules/generator.py): appearance encoder -> dense motion field -> warp every skip ->
concat key-point heat-maps -> decoder -> residual refinement -> 1x1 conv + sigmoid; all on the gfx950 kernels."""
import torch
from torch import nn

from modules.util import Encoder, Decoder, ResBlock3D
from modules.dense_motion_module import DenseMotionModule, IdentityDeformation
from modules.movement_embedding import MovementEmbeddingModule
from mnk import ops

_MODES = {'nearest': 0, 'trilinear': 1}


class SourceState:
    """What MotionTransferGenerator.encode_source keeps of one batch of source images: the appearance encoder's skip acts
    [(act, channels)], the source as an act, and the down-scaled source acts the two movement embeddings read when they use the
    deformed source image (None where they do not); B, H, W of the source."""
    __slots__ = ("skips", "src_act", "mask_src", "emb_src", "B", "H", "W")

    def __init__(self, skips, src_act, mask_src, emb_src, B, H, W):
        self.skips, self.src_act, self.mask_src, self.emb_src = skips, src_act, mask_src, emb_src
        self.B, self.H, self.W = B, H, W

    def tensors(self):
        out = [a for a, _ in self.skips] + [self.src_act, self.mask_src, self.emb_src]
        seen, uniq = set(), []
        for t in out:                        # (the first skip IS the source act)
            if t is not None and id(t) not in seen:
                seen.add(id(t))
                uniq.append(t)
        return uniq

    def copy_from(self, other):
        """take another state's values in place (same shapes): captured programs that read this state stay valid"""
        mine, theirs = self.tensors(), other.tensors()
        if len(mine) != len(theirs) or any(a.shape != b.shape for a, b in zip(mine, theirs)):
            raise ValueError("source states of different shapes")
        for a, b in zip(mine, theirs):
            a.copy_(b)


class MotionTransferGenerator(nn.Module):
    """Given key-points and a source frame, reconstruct the driving frames.  Returns the refined prediction and the
    purely warped source (generator.py:10-82), both (B, C, d, H, W) for d driving frames per source (output="uint8": both as uint8
    (B, d, H, W, C) frames, `(255 * out).astype(np.uint8)` channel-last as demo.py:69-71 saves them): the source is encoded
    once (B rows), the field, the embedding, the decoder and the refinement run on the B*d rows v*d + f, and the warps read
    source row v for every frame of video v (the reference's grid_sample over a depth-1 volume, generator.py:51-58)."""

    def __init__(self, num_channels, num_kp, kp_variance, block_expansion, max_features, num_blocks, num_refinement_blocks,
                 dense_motion_params=None, kp_embedding_params=None, interpolation_mode='nearest'):
        super(MotionTransferGenerator, self).__init__()
        self.appearance_encoder = Encoder(block_expansion, in_features=num_channels, max_features=max_features,
                                          num_blocks=num_blocks)
        if kp_embedding_params is not None:
            self.kp_embedding_module = MovementEmbeddingModule(num_kp=num_kp, kp_variance=kp_variance,
                                                               num_channels=num_channels, **kp_embedding_params)
            embedding_features = self.kp_embedding_module.out_channels
        else:
            self.kp_embedding_module = None
            embedding_features = 0
        if dense_motion_params is not None:
            self.dense_motion_module = DenseMotionModule(num_kp=num_kp, kp_variance=kp_variance,
                                                         num_channels=num_channels, **dense_motion_params)
        else:
            self.dense_motion_module = IdentityDeformation()
        self.video_decoder = Decoder(block_expansion=block_expansion, in_features=num_channels,
                                     out_features=num_channels, max_features=max_features, num_blocks=num_blocks,
                                     additional_features_for_block=embedding_features, use_last_conv=False)
        self.refinement_module = torch.nn.Sequential()
        in_features = block_expansion + num_channels + embedding_features
        for i in range(num_refinement_blocks):
            self.refinement_module.add_module('r' + str(i), ResBlock3D(in_features, kernel_size=(1, 3, 3),
                                                                       padding=(0, 1, 1)))
        self.refinement_module.add_module('conv-last', nn.Conv3d(in_features, num_channels, kernel_size=1, padding=0))
        self.interpolation_mode = interpolation_mode
        self.num_channels = num_channels
        self.refine_features = in_features

    def _mode(self):
        if self.interpolation_mode not in _MODES:
            raise NotImplementedError("interpolation_mode %r" % (self.interpolation_mode,))
        return _MODES[self.interpolation_mode]

    def deform_input(self, inp, deformations_absolute):
        """Public form of generator.py:51-58: inp (B,C,1,h,w), field (B,d,ho,wo,3) -> (B,C,d,h,w)."""
        b, c = inp.shape[:2]
        _, d, ho, wo, _ = deformations_absolute.shape
        if inp.shape[2] != 1:
            raise NotImplementedError("deform_input takes one source frame per video; got %d" % inp.shape[2])
        field = deformations_absolute[..., :2].reshape(b * d, ho, wo, 2).contiguous()
        out = ops.WarpSkipFn.apply(ops.to_act(inp), field, None, c, 0, self._mode())
        return ops.from_act(out, c, b)

    @torch.no_grad()
    def encode_source(self, source_image):
        """Everything forward() computes from the source image alone, for callers that generate from one source over several
        calls (mnk.engine.AnimationSession): -> SourceState.  Evaluation mode only (a training-mode BatchNorm of the encoder
        would need the batch of every call).  The state holds activations, not weights: encode again after the weights change."""
        if self.training:
            raise RuntimeError("encode_source works in evaluation mode: the appearance encoder's BatchNorm layers would take "
                               "their statistics from this call's batch")
        if ops.is_u8(source_image):
            ops.require_inference(self, source_image)
        if source_image.dim() != 5 or source_image.shape[2] != 1:
            raise NotImplementedError("the generator takes one source frame per video; got a source of shape %s"
                                      % (tuple(source_image.shape),))
        b, _, _, h, w = source_image.shape
        src_act = ops.to_act(source_image)
        skips = self.appearance_encoder.forward_act(src_act, self.num_channels)
        state = SourceState(skips, src_act, None, None, b, h, w)
        dm = self.dense_motion_module
        if isinstance(dm, DenseMotionModule) and dm.mask_embedding.use_deformed_source_image:
            state.mask_src = ops.to_act(source_image, ops.step_from_scale(dm.mask_embedding.scale_factor)
                                        * ops.step_from_scale(dm.scale_factor))
        if self.kp_embedding_module is not None and self.kp_embedding_module.use_deformed_source_image:
            state.emb_src = ops.to_act(source_image, ops.step_from_scale(self.kp_embedding_module.scale_factor))
        # every tensor of the state is finished: no split-K partial sum or norm hand-over of mnk.ops may point into it
        # (the encoder ends in a norm layer, which takes both)
        pending = ops.pending_outputs()
        if any(t.data_ptr() in pending for t in state.tensors()):
            raise RuntimeError("encode_source: an activation of the state still waits for its norm layer")
        return state

    def forward(self, source_image, kp_driving, kp_source, source_state=None, output="float"):
        """source_state: what encode_source(source_image) returned -- the encoder and the source's layout conversions are skipped
        (evaluation mode; `source_image` then only gives the shapes).  None: everything is computed here.
        source_image: (B, C, 1, H, W) fp32 or ops.U8Frames (uint8 channel-last, evaluation mode without gradients).
        output: "float" -- fp32 (B, C, d, H, W); "uint8" -- uint8 (B, d, H, W, C) written by the last kernels themselves (the fp32
        tensors are not made); evaluation mode under torch.no_grad() only."""
        if ops.check_output(output) == "uint8":
            if self.training or torch.is_grad_enabled():
                raise RuntimeError('output="uint8" carries no gradient: call .eval() and wrap the call in torch.no_grad() '
                                   '(or keep output="float")')
        if ops.is_u8(source_image):
            ops.require_inference(self, source_image)
        if source_state is not None:
            return self._forward_from_state(source_image, kp_driving, kp_source, source_state, output)
        b = source_image.shape[0]
        d = kp_driving['mean'].shape[1]
        if d < 1 or source_image.shape[2] != 1:
            raise NotImplementedError("the generator takes one source frame per video (train.py:38, reconstruction.py:15-17, "
                                      "transfer.py:72-74) and d >= 1 driving frames; got %d source frames, d = %d"
                                      % (source_image.shape[2], d))
        mode = self._mode()
        src_act = ops.to_act(source_image)
        # (the appearance encoder does not depend on the key points; running it as a second-stream branch next to the
        # dense-motion network was measured at 11.46 vs 11.44 ms per step -- every kernel fills the chip -- and removed)
        skips = self.appearance_encoder.forward_act(src_act, self.num_channels)
        field = self.dense_motion_module.field_act(source_image, kp_driving, kp_source)     # (B*d,hf,wf,2)
        emb, ke = None, 0
        if self.kp_embedding_module is not None:
            emb, ke = self.kp_embedding_module.forward_act(source_image, kp_driving, kp_source)
        # all warps of this forward as one autograd node: one shared field-gradient buffer (ops.WarpAllFn); the B source
        # rows are shared by the d frames of their video, the outputs have B*d rows
        return self._decode(b, field, emb, ke, mode, skips, src_act, output)

    def _forward_from_state(self, source_image, kp_driving, kp_source, state, output="float"):
        if self.training:
            raise RuntimeError("a source state serves evaluation mode only: in training mode the appearance encoder's BatchNorm "
                               "layers take their statistics from the batch, so the encoder has to run")
        b, d = source_image.shape[0], kp_driving['mean'].shape[1]
        if d < 1 or source_image.shape[2] != 1:
            raise NotImplementedError("the generator takes one source frame per video and d >= 1 driving frames; got %d source "
                                      "frames, d = %d" % (source_image.shape[2], d))
        if (b,) + tuple(source_image.shape[3:]) != (state.B, state.H, state.W):
            raise ValueError("the source state was encoded for (B, H, W) = %s, the source image has %s"
                             % ((state.B, state.H, state.W), (b,) + tuple(source_image.shape[3:])))
        mode = self._mode()
        if isinstance(self.dense_motion_module, DenseMotionModule):
            field = self.dense_motion_module.field_act(source_image, kp_driving, kp_source, src_act=state.mask_src)
        else:
            field = self.dense_motion_module.field_act(source_image, kp_driving, kp_source)
        emb, ke = None, 0
        if self.kp_embedding_module is not None:
            emb, ke = self.kp_embedding_module.forward_act(source_image, kp_driving, kp_source, src_act=state.emb_src)
        return self._decode(b, field, emb, ke, mode, state.skips, state.src_act, output)

    def _decode(self, b, field, emb, ke, mode, skips, src_act, output="float"):
        specs = tuple((c, ke) for _, c in skips) + ((self.num_channels, 0),)
        outs = ops.WarpAllFn.apply(field, emb, mode, specs, *([a for a, _ in skips] + [src_act]))
        warped = [(o, c + ke) for o, (_, c) in zip(outs[:-1], skips)]
        deformed_img = outs[-1]
        u8 = output == "uint8"
        video_deformed = ops.act_to_u8(deformed_img, self.num_channels, b) if u8 else ops.from_act(deformed_img, self.num_channels, b)
        out, c = self.video_decoder.forward_act(warped)
        last, sums = None, None
        blocks = list(self.refinement_module.named_children())
        for idx, (name, block) in enumerate(blocks):
            if name == 'conv-last':
                last = block
            else:     # hand the output statistics of each block to the next block's norm1 (fused in the conv epilogue)
                more = idx + 1 < len(blocks) and blocks[idx + 1][0] != 'conv-last' and block.training
                res = block.forward_act(out, c, x_sums=sums, want_stats=more)
                out, c = res[0], res[1]
                sums = res[2] if more else None
        if u8:
            video_prediction = ops.conv1x1_sigmoid_u8(out, last.weight, last.bias, c, b)
        else:
            video_prediction = ops.Conv1x1SigmoidFn.apply(out, last.weight, last.bias, c, b)
        return {"video_prediction": video_prediction, "video_deformed": video_deformed}
