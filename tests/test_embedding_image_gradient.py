"""Gradient of the source image through MovementEmbeddingModule with use_deformed_source_image (movement_embedding.py:76-87:
the image is sampled once per frame and key-point slot, translated by kp_source - kp_driving), and through the nearest
down-scaling in front of it (movement_embedding.py:43-44).  No caller of the reference asks for it, the multi-frame generator
tests do: mnk_movement_embedding_img_bwd (a gather per image texel over the d frames of its video) and
mnk_nhwc_to_ncdhw_strided, against the fp64 autograd of oracle.restate.movement_embedding."""
import pytest
import torch

from _util import relerr
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from oracle import cases, restate

# the embedding variants of oracle/make_golden.py that read the image, at one and three driving frames, full and half size,
# small and large translations (spread 1.2: many samples fall outside the image)
VARIANTS = {
    "mask": dict(use_heatmap=True, use_deformed_source_image=True, heatmap_type="difference", norm_const=100,
                 add_bg_feature_map=True),
    "mask_diff": dict(use_heatmap=True, use_deformed_source_image=True, use_difference=True, heatmap_type="difference",
                      norm_const=100, add_bg_feature_map=True),
    "sum_no_bg": dict(use_heatmap=True, use_deformed_source_image=True, heatmap_type="gaussian", norm_const="sum"),
    "image_only": dict(use_heatmap=False, use_deformed_source_image=True),
}
CASES = [("mask", 1, 1, (16, 16), 0.6), ("mask_diff", 3, 1, (16, 12), 0.6), ("sum_no_bg", 3, 0.5, (32, 24), 0.6),
         ("image_only", 2, 1, (9, 13), 1.2), ("mask", 3, 0.5, (34, 30), 1.2)]


@pytest.mark.parametrize("tag,d,scale,hw,spread", CASES)
def test_source_image_gradient_of_the_movement_embedding(be, tag, d, scale, hw, spread):
    from modules.movement_embedding import MovementEmbeddingModule
    g = torch.Generator().manual_seed(8)
    b, k, c = 2, 4, 3
    kw = dict(VARIANTS[tag], scale_factor=scale)
    src = torch.rand(b, c, 1, hw[0], hw[1], generator=g)
    kp_d, kp_s = cases.random_kp(b, d, k, seed=6, spread=spread), cases.random_kp(b, 1, k, seed=7, spread=spread)
    s64 = src.double().requires_grad_(True)
    ref = restate.movement_embedding(dict(kw, num_kp=k, kp_variance="matrix", num_channels=c), s64,
                                     {n: v.double() for n, v in kp_d.items()}, {n: v.double() for n, v in kp_s.items()})
    w = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    (ref * w).sum().backward()
    mod = MovementEmbeddingModule(num_kp=k, kp_variance="matrix", num_channels=c, **kw)
    runs = []
    for _ in range(2):
        x = be.t(src).requires_grad_(True)
        out = mod(x, {n: be.t(v) for n, v in kp_d.items()}, {n: be.t(v) for n, v in kp_s.items()})
        (out * be.t(w.float())).sum().backward()
        be.sync()
        runs.append(x.grad.cpu())
    assert float((out.detach().cpu().double() - ref.detach()).abs().max()) < 1e-5
    assert runs[0].shape == src.shape
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))       # a fixed summation order
    err = relerr(runs[0], s64.grad)
    print("%s d=%d scale=%s: relerr(d source) = %.3e" % (tag, d, scale, err))
    # fp32 sums of at most d * (K + 1) * 4 products per texel against fp64: a few 1e-7; the bound of test_deform
    assert err < 1e-5
    if scale != 1:          # the pixels the down-scaling does not pick get exactly 0
        step = int(round(1 / scale))
        mask = torch.ones(hw, dtype=torch.bool)
        mask[::step, ::step] = False
        assert torch.all(runs[0][..., mask] == 0) and torch.all(s64.grad[..., mask] == 0)


def test_strided_layout_adjoint_writes_every_element(be):
    g = torch.Generator().manual_seed(3)
    b, c, d, h, w, step = 2, 3, 2, 9, 10, 2
    ho, wo, ld = h // step, w // step, 4
    act = torch.randn(b * d, ho, wo, ld, generator=g)
    out = be.empty(b, c, d, h, w)
    be.call("mnk_nhwc_to_ncdhw_strided", be.t(act), ld, out, b, c, d, h, w, step)
    be.sync()
    want = torch.zeros(b, c, d, h, w)
    want[..., :ho * step:step, :wo * step:step] = act[..., :c].view(b, d, ho, wo, c).permute(0, 4, 1, 2, 3)
    assert torch.equal(out.cpu(), want)
