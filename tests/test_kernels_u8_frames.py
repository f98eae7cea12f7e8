"""The uint8 frame kernels: mnk_u8_to_nhwc (frames_dataset.py:14-29 fused with the layout conversion), mnk_conv1x1_fwd_u8 (the
generator's conv-last + sigmoid with `(255 * out).astype(np.uint8)` as its epilogue, demo.py:69-71) and mnk_nhwc_to_u8.

Every expected value is computed in torch on the host; all comparisons are exact (bits / bytes): the kernels do one fp32 product
per value (float(byte) * (1.f / 255.f), 255.f * x) and no sum of their own -- the 1x1 kernels are the fp32 entry's kernels with
another epilogue, and are compared with that entry on the same buffers.  Buffers are guard-banded (tests/_guard.py)."""
import pytest
import torch

from _guard import be  # noqa: F401  (guard-banded buffers, checked calls; emu + hip)

K255 = torch.tensor(1.0 / 255.0, dtype=torch.float32)


def bits(t):
    return t.contiguous().cpu().view(torch.int32)


def _bytes(shape, mult=73, add=5):
    """a uint8 tensor whose flat values walk all 256 byte values (mult is odd): different in every neighbouring pixel"""
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n, dtype=torch.int64) * mult + add) % 256).to(torch.uint8).view(shape)


def _rgb_float(u8):
    """(B, D, H, W, Cs) uint8 -> the fp32 (B, 3, D, H, W) tensor read_video + VideoToTensor give (frames_dataset.py:14-29)"""
    rgb = u8.expand(-1, -1, -1, -1, 3) if u8.shape[4] == 1 else u8[..., :3]
    return (rgb.permute(0, 4, 1, 2, 3).float() * K255).contiguous()


def _expected_act(x5, step, ld):
    b, c, d, h, w = x5.shape
    ho, wo = h // step, w // step
    picked = x5[:, :, :, :ho * step:step, :wo * step:step]
    out = torch.zeros(b * d, ho, wo, ld, dtype=torch.float32)
    out[..., :c] = picked.permute(0, 2, 3, 4, 1).reshape(b * d, ho, wo, c)
    return out


SHAPES = [(2, 3, 5, 7), (1, 1, 8, 12), (1, 2, 33, 65)]


@pytest.mark.parametrize("cs", [1, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=["2x3x5x7", "1x1x8x12", "1x2x33x65"])
def test_u8_to_nhwc_equals_the_float_conversion_bit_for_bit(be, shape, cs):
    b, d, h, w = shape
    host = _bytes((b, d, h, w, cs))
    if (b, d, h, w) == SHAPES[2]:
        assert len(torch.unique(host)) == 256                        # one input holds every byte value
    x5 = _rgb_float(host)
    src, src5 = be.t(host), be.t(x5)
    forms = set()
    for step in (1, 2, 4):
        if h // step < 1 or w // step < 1:
            continue
        for ld in (4, 8):
            want = _expected_act(x5, step, ld)
            got = be.empty(*want.shape)
            be.call("mnk_u8_to_nhwc", src, got, b, d, h, w, cs, step, ld)
            assert torch.equal(bits(got), bits(want)), (shape, cs, step, ld)
            # ... and that IS mnk_ncdhw_to_nhwc of the fp32 tensor of those values, pad lanes included
            ref = be.empty(*want.shape)
            be.call("mnk_ncdhw_to_nhwc", src5, ref, b, 3, d, h, w, step, ld)
            assert torch.equal(bits(got), bits(ref)), (shape, cs, step, ld)
            forms.add("rgb4" if cs == 3 and step == 1 and (b * d * h * w) % 4 == 0 else ("dword" if cs == 4 else "bytes"))
    print("forms run:", sorted(forms))
    if cs == 3:                 # the pixel count decides at step 1: 96 pixels take the dword form, 210 and 4290 the byte form
        assert ("rgb4" in forms) == ((b * d * h * w) % 4 == 0)


def test_u8_to_nhwc_never_reads_alpha_into_the_result(be):
    b, d, h, w = 2, 3, 5, 7
    a = _bytes((b, d, h, w, 4))
    a[..., 3] = _bytes((b, d, h, w), mult=57, add=3)                 # a different alpha in every pixel
    other = a.clone()
    other[..., 3] = _bytes((b, d, h, w), mult=91, add=17)            # another alpha in every pixel
    assert not torch.equal(a[..., 3], other[..., 3]) and len(torch.unique(a[..., 3])) > 100
    want = _expected_act(_rgb_float(a), 1, 4)
    for host in (a, other):
        got = be.empty(*want.shape)
        be.call("mnk_u8_to_nhwc", be.t(host), got, b, d, h, w, 4, 1, 4)
        assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("cs", [3, 4])
def test_u8_to_nhwc_from_a_source_one_byte_off_a_dword(be, cs):
    b, d, h, w = 1, 1, 8, 12                                         # W * Cs % 4 == 0: only the address forbids the dword loads
    host = _bytes((b, d, h, w, cs), mult=29)
    buf = be.t(torch.cat([torch.zeros(1, dtype=torch.uint8), host.reshape(-1)]))
    src = buf[1:].view(b, d, h, w, cs)
    assert src.data_ptr() % 4 == 1
    for step in (1, 2):
        want = _expected_act(_rgb_float(host), step, 4)
        got = be.empty(*want.shape)
        be.call("mnk_u8_to_nhwc", src, got, b, d, h, w, cs, step, 4)
        assert torch.equal(bits(got), bits(want)), (cs, step)


# (ld_x, Cin): one case per forward form of mnk_conv1x1_fwd -- the row-tile form (ld_x % 4 == 0, <= 64), the wave-per-row form
# (Cin >= 64 where the row-tile form does not apply) and the thread-per-pixel form
FORMS = [(48, 45), (68, 66), (6, 5)]


@pytest.mark.parametrize("cout", [1, 3])
@pytest.mark.parametrize("ld_x,cin", FORMS, ids=["rows", "wave", "pixel"])
def test_conv1x1_u8_bytes_are_the_truncated_fp32_outputs(be, ld_x, cin, cout):
    b, d, h, w = 2, 3, 5, 7
    rows = b * d * h * w                                             # 210: a full and a partial 128-row tile
    g = torch.Generator().manual_seed(100 * ld_x + cout)
    x = torch.zeros(rows, ld_x)
    x[:, :cin] = torch.randn(rows, cin, generator=g)
    wt = torch.randn(cout, cin, generator=g) * (4.0 / cin ** 0.5)    # pre-activations of about +-8 in every channel
    bias = torch.randn(cout, generator=g)
    # channel 0 walks the bytes: its pre-activation in row r is logit((j_r + 0.5) / 255), j_r = 210 distinct values of 0 .. 254
    # (the middle of byte j_r: +-6.2), made by solving for x[r, 0] with w[0, 0] = 1
    wt[0, 0] = 1.0
    j = torch.round(torch.arange(rows, dtype=torch.float64) * 254.0 / (rows - 1))
    p = (j + 0.5) / 255.0
    rest = x[:, 1:cin].double() @ wt[0, 1:].double() + bias[0].double()
    x[:, 0] = (torch.log(p / (1 - p)) - rest).float()
    xd, wd, bd = be.t(x), be.t(wt), be.t(bias)
    ref = be.empty(b, cout, d, h, w)
    be.call("mnk_conv1x1_fwd", xd, ld_x, cin, wd, bd, ref, b, d, h, w, cout, 1)
    got = be.empty_int(b, d, h, w, cout, dtype=torch.uint8)
    be.call("mnk_conv1x1_fwd_u8", xd, ld_x, cin, wd, bd, got, b, d, h, w, cout)
    want = (255 * ref.cpu()).to(torch.uint8).permute(0, 2, 3, 4, 1).contiguous()
    distinct = len(torch.unique(want))
    print("ld_x %d Cin %d Cout %d: %d distinct byte values, %d .. %d" % (ld_x, cin, cout, distinct, int(want.min()), int(want.max())))
    assert distinct >= 200
    assert torch.equal(got.cpu(), want)
    # the fp32 entry is what it was: the chain bias, then += x[k] * w[k] in the order of its form
    err = float((ref.cpu() - torch.sigmoid(x[:, :cin].double() @ wt.double().t() + bias.double()).float()
                 .view(b, d, h, w, cout).permute(0, 4, 1, 2, 3)).abs().max())
    assert err < 1e-5, err


def test_conv1x1_u8_into_an_unaligned_output(be):
    """an output one byte off a dword: the block pieces go out by bytes"""
    ld_x, cin, cout, (b, d, h, w) = 48, 45, 3, (2, 3, 5, 7)
    g = torch.Generator().manual_seed(5)
    x, wt, bias = torch.randn(b * d * h * w, ld_x, generator=g), torch.randn(cout, cin, generator=g) * 0.6, torch.randn(cout, generator=g)
    xd, wd, bd = be.t(x), be.t(wt), be.t(bias)
    ref = be.empty(b, cout, d, h, w)
    be.call("mnk_conv1x1_fwd", xd, ld_x, cin, wd, bd, ref, b, d, h, w, cout, 1)
    buf = be.empty_int(b * d * h * w * cout + 1, dtype=torch.uint8)
    got = buf[1:].view(b, d, h, w, cout)
    be.call("mnk_conv1x1_fwd_u8", xd, ld_x, cin, wd, bd, got, b, d, h, w, cout)
    assert torch.equal(got.cpu(), (255 * ref.cpu()).to(torch.uint8).permute(0, 2, 3, 4, 1))
    assert int(buf[0]) == 0x5A


@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("rows", [1, 210, 4097])
def test_nhwc_to_u8(be, rows, ld):
    g = torch.Generator().manual_seed(rows + ld)
    x = torch.rand(rows, ld, generator=g)
    x[0, :3] = torch.tensor([0.0, 1.0, 254.0 / 255.0])               # the ends of the range and a value at a byte's edge
    if rows > 4:
        x[1:4, :3] = (torch.arange(9, dtype=torch.float32).view(3, 3) * 31 + 3) * K255
    x[:, 3:] = 7.0                                                   # the pad lanes are not read
    want = (255 * x[:, :3]).to(torch.uint8)
    got = be.empty_int(rows, 3, dtype=torch.uint8)
    be.call("mnk_nhwc_to_u8", be.t(x), ld, got, rows, 3)
    assert torch.equal(got.cpu(), want)
    buf = be.empty_int(rows * 3 + 1, dtype=torch.uint8)              # one byte off a dword: the byte form
    be.call("mnk_nhwc_to_u8", be.t(x), ld, buf[1:], rows, 3)
    assert torch.equal(buf[1:].cpu().view(rows, 3), want) and int(buf[0]) == 0x5A


def test_rejected_arguments_raise_and_leave_the_guards_intact(be):
    from mnk._lib import MnkError
    b, d, h, w = 1, 2, 4, 4
    src = be.t(_bytes((b, d, h, w, 4)))
    dst = be.empty(b * d, h, w, 4)
    for cs, step, ld in ((2, 1, 4), (0, 1, 4), (5, 1, 4), (3, 0, 4), (3, -1, 4), (3, 1, 2), (3, 8, 4)):
        with pytest.raises(MnkError, match="invalid argument"):
            be.call("mnk_u8_to_nhwc", src, dst, b, d, h, w, cs, step, ld)
    for s, o in ((None, dst), (src, None)):
        with pytest.raises(MnkError, match="invalid argument"):
            be.call("mnk_u8_to_nhwc", s, o, b, d, h, w, 3, 1, 4)
    assert torch.isnan(dst).all()
    rows = b * d * h * w
    x, wt, bias = be.t(torch.randn(rows, 8)), be.t(torch.randn(5, 6)), be.t(torch.randn(5))
    out = be.empty_int(rows, 5, dtype=torch.uint8)
    for cin, cout, ld_x in ((6, 5, 8), (6, 0, 8), (0, 3, 8), (6, 3, 4)):     # Cout over the limit of 4, empty, ld_x < Cin
        with pytest.raises(MnkError, match="invalid argument"):
            be.call("mnk_conv1x1_fwd_u8", x, ld_x, cin, wt, bias, out, b, d, h, w, cout)
    for xx, ww, oo in ((None, wt, out), (x, None, out), (x, wt, None)):
        with pytest.raises(MnkError, match="invalid argument"):
            be.call("mnk_conv1x1_fwd_u8", xx, 8, 6, ww, bias, oo, b, d, h, w, 3)
    for args in ((None, 8, out, rows, 3), (x, 8, None, rows, 3), (x, 8, out, 0, 3), (x, 8, out, rows, 0), (x, 2, out, rows, 3)):
        with pytest.raises(MnkError, match="invalid argument"):
            be.call("mnk_nhwc_to_u8", *args)
    assert bool((out.cpu() == 0x5A).all())
