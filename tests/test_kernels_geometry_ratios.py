"""Resize, warp and layout kernels off the power-of-two grid.

The geometry kernels compute a source index in fp32 and a gather window in integers; the two must agree at every size the
product can meet (the generator's level sizes are floor(H / 2^k): a frame of 80 gives 5 -> 2, one of 100 gives 12).  Here:
non-integer and non-square ratios, the size pairs at which the fp32 nearest pick is not floor(dst * in / out) -- the only sizes
at which the integer windows and the float index disagree by one --, one-texel axes, windows wider than 16 pixels, grids
beyond one pass of the layout kernels' grid-stride loops, and strided layout copies whose step does not divide the frame.

Tolerances are measured (_util.within): outputs that are picks or copies are compared exactly; every other output must lie
within max(the project's bound, 4 x the error of the same reference computed in fp32 by stock torch) of the fp64 reference."""
import pytest
import torch
import torch.nn.functional as F

from _util import to_nhwc, from_nhwc, ceil4, relerr, maxerr, within
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from _warp_levels import WARP_TABLES_RATIOS, identity_field, run_warp_levels
from oracle import restate

# (in, out) <= 64 at which floorf(dst * ((float)in / (float)out)) != floor(dst * in / out) for some dst
FLOAT_VS_RATIONAL = {(14, 46), (26, 22), (26, 44), (28, 46), (30, 58), (39, 33), (52, 22), (52, 44), (54, 38), (56, 46),
                     (58, 54), (60, 58), (62, 14), (62, 28), (62, 56)}

# (source or field h, w) -> (map h, w)
POOL = [
    ((26, 14), (22, 46)), ((62, 39), (14, 33)), ((52, 54), (22, 38)), ((14, 62), (46, 28)),             # float vs rational
    ((7, 5), (3, 4)), ((5, 9), (13, 7)), ((25, 25), (12, 12)), ((12, 10), (5, 3)), ((13, 11), (4, 6)),  # non-integer ratios
    ((10, 6), (3, 1)), ((1, 3), (5, 7)),                                                                # one-texel axes
    ((6, 5), (100, 37)), ((3, 3), (50, 50)), ((4, 4), (80, 9)),                                         # wide windows
]
POOL_IDS = ["%dx%d-to-%dx%d" % (a + b) for a, b in POOL]
RESIZE_BOUND = 2e-6           # test_resize_bilinear's forward tolerance
DEFORM_BOUND = 1e-5           # test_deform's


def test_nearest_index_is_the_float32_pick():
    """restate.nearest_index == F.interpolate(float32, 'nearest') along both axes, 4-D and 5-D, for every in, out <= 64; and
    it differs from the rational floor(dst * in / out) at exactly FLOAT_VS_RATIONAL (the pool's first row comes from it)."""
    differ = set()
    for i in range(1, 65):
        x = (torch.arange(i).view(i, 1) * i + torch.arange(i).view(1, i)).float()
        for o in range(1, 65):
            idx = restate.nearest_index(i, o)
            assert idx.dtype == torch.long and idx.shape == (o,) and int(idx.max()) <= i - 1
            want = (idx.view(o, 1) * i + idx.view(1, o)).float()
            assert torch.equal(F.interpolate(x.view(1, 1, i, i), size=(o, o), mode="nearest")[0, 0], want), (i, o)
            assert torch.equal(F.interpolate(x.view(1, 1, 1, i, i), size=(1, o, o), mode="nearest")[0, 0, 0], want), (i, o)
            if not torch.equal(idx, torch.arange(o) * i // o):
                differ.add((i, o))
    assert differ == FLOAT_VS_RATIONAL, sorted(differ ^ FLOAT_VS_RATIONAL)
    for (hs, ws), (hd, wd) in POOL[:4]:
        assert (hs, hd) in FLOAT_VS_RATIONAL or (ws, wd) in FLOAT_VS_RATIONAL


def test_resize_field_picks_the_float32_texel_in_every_dtype():
    """restate.resize_field(mode='nearest') on fp64 == on fp32, at a pair where ATen's own fp64 5-D pick is another texel"""
    g = torch.Generator().manual_seed(1)
    f = torch.randn(2, 1, 26, 14, 3, generator=g)
    a, b = restate.resize_field(f, (22, 46), "nearest"), restate.resize_field(f.double(), (22, 46), "nearest")
    assert a.shape == (2, 1, 22, 46, 3) and torch.equal(a.double(), b)
    ref = F.interpolate(f.permute(0, 4, 1, 2, 3), size=(1, 22, 46), mode="nearest").permute(0, 2, 3, 4, 1)
    assert torch.equal(a, ref)


# ---- 1. resize kernels -------------------------------------------------------------------------------------------------------
def _columns(n, h, w, ld, off, x4):
    """(n, h, w, ld) of NaN with x4 (n, c, h, w) in channels [off, off + c): whatever else is read poisons the result"""
    t = torch.full((n, h, w, ld), float("nan"))
    t[..., off:off + x4.shape[1]] = x4.permute(0, 2, 3, 1)
    return t


@pytest.mark.parametrize("src,dst", POOL, ids=POOL_IDS)
def test_resize_nearest_off_grid(be, src, dst):
    """mnk_resize_nearest (bit for bit the fp32 F.interpolate), _bwd and _bwd_accumulate (on a non-zero buffer: previous +
    gradient) against fp64 autograd of the same pick; dst_off = 2, ld_dst = 8 > C + dst_off, the other columns NaN"""
    (hs, ws), (hd, wd) = src, dst
    g = torch.Generator().manual_seed(2)
    n, c, lds, ldd, off = 2, 3, 4, 8, 2
    s = torch.randn(n, c, hs, ws, generator=g)
    dd = torch.randn(n, c, hd, wd, generator=g)
    prev = torch.randn(n, hs, ws, lds, generator=g)
    s32 = s.clone().requires_grad_(True)
    ref = F.interpolate(s32, size=(hd, wd), mode="nearest")
    ref.backward(dd)
    s64 = s.double().requires_grad_(True)
    pick = s64[:, :, restate.nearest_index(hs, hd)][:, :, :, restate.nearest_index(ws, wd)]
    assert torch.equal(pick.detach(), ref.detach().double())
    pick.backward(dd.double())
    S, O = be.t(to_nhwc(s)), be.empty(n, hd, wd, ldd)
    be.call("mnk_resize_nearest", S, lds, hs, ws, O, ldd, off, hd, wd, n, c)
    DD = be.t(_columns(n, hd, wd, ldd, off, dd))
    DS, DSA = be.empty(n, hs, ws, lds), be.t(prev)
    be.call("mnk_resize_nearest_bwd", DD, ldd, off, hd, wd, DS, lds, hs, ws, n, c)
    be.call("mnk_resize_nearest_bwd_accumulate", DD, ldd, off, hd, wd, DSA, lds, hs, ws, n, c)
    be.sync()
    o, ds, dsa = O.cpu(), DS.cpu(), DSA.cpu()
    assert torch.equal(o[..., off:off + c].permute(0, 3, 1, 2), ref.detach())
    assert torch.isnan(o[..., :off]).all() and torch.isnan(o[..., off + c:]).all()
    label = "resize-nearest %s [%s] " % (POOL_IDS[POOL.index((src, dst))], be.kind)
    assert within(label + "dsrc", maxerr, from_nhwc(ds, c), s64.grad, s32.grad, RESIZE_BOUND)[0]
    p4 = prev[..., :c].permute(0, 3, 1, 2)
    assert within(label + "dsrc-accumulated", maxerr, from_nhwc(dsa, c), p4.double() + s64.grad, p4 + s32.grad, RESIZE_BOUND)[0]
    assert torch.isnan(ds[..., c:]).all() and torch.equal(dsa[..., c:], prev[..., c:])


@pytest.mark.parametrize("src,dst", POOL, ids=POOL_IDS)
def test_resize_bilinear_off_grid(be, src, dst):
    """mnk_resize_bilinear / _bwd (added to a non-zero buffer) against fp64 F.interpolate(bilinear, align_corners=False) and
    its autograd; the same offsets as above"""
    (hs, ws), (hd, wd) = src, dst
    g = torch.Generator().manual_seed(5)
    n, c, lds, ldd, off = 2, 3, 4, 8, 2
    s = torch.randn(n, c, hs, ws, generator=g)
    dd = torch.randn(n, c, hd, wd, generator=g)
    prev = torch.randn(n, hs, ws, lds, generator=g)
    refs = []
    for dtype in (torch.float64, torch.float32):
        sr = s.to(dtype).requires_grad_(True)
        r = F.interpolate(sr, size=(hd, wd), mode="bilinear", align_corners=False)
        r.backward(dd.to(dtype))
        refs.append((r.detach(), sr.grad))
    (r64, g64), (r32, g32) = refs
    S, O = be.t(to_nhwc(s)), be.empty(n, hd, wd, ldd)
    be.call("mnk_resize_bilinear", S, lds, hs, ws, O, ldd, off, hd, wd, n, c)
    DD, DS = be.t(_columns(n, hd, wd, ldd, off, dd)), be.t(prev)
    be.call("mnk_resize_bilinear_bwd", DD, ldd, off, hd, wd, DS, lds, hs, ws, n, c)
    be.sync()
    o, ds = O.cpu(), DS.cpu()
    label = "resize-bilinear %s [%s] " % (POOL_IDS[POOL.index((src, dst))], be.kind)
    assert within(label + "out", maxerr, o[..., off:off + c].permute(0, 3, 1, 2), r64, r32, RESIZE_BOUND)[0]
    assert torch.isnan(o[..., :off]).all() and torch.isnan(o[..., off + c:]).all()
    p4 = prev[..., :c].permute(0, 3, 1, 2)
    assert within(label + "dsrc", maxerr, from_nhwc(ds, c), p4.double() + g64, p4 + g32, RESIZE_BOUND)[0]
    assert torch.equal(ds[..., c:], prev[..., c:])


# ---- 2. deform -----------------------------------------------------------------------------------------------------------------
def _clear_of_texel_boundaries(field, h, w, mode):
    """d out / d field jumps where a sampling point crosses a texel boundary: a point that the rounding of the coordinate
    arithmetic can move across one makes the fp32 and the fp64 reference differ by a whole term, and 4 x that is no tolerance.
    True if every sampling coordinate of the fp64 reference (texel units, grid_sample's ((x + 1) / 2) * (size - 1)) is further
    from an integer than 4 x the largest difference between the fp32 and the fp64 reference's coordinates.  References only:
    the kernels have no part in it.  (An axis of one texel has the coordinate 0 in every arithmetic.)"""
    name, cs = "nearest" if mode == 0 else "trilinear", []
    for dtype in (torch.float64, torch.float32):
        f = restate.resize_field(field.to(dtype), (h, w), name)[..., :2]
        cs.append((((f + 1) / 2) * torch.tensor([w - 1, h - 1], dtype=dtype)).double())
    axes = torch.tensor([w > 1, h > 1])
    c64, c32 = cs[0][..., axes], cs[1][..., axes]
    return bool(((c64 - c64.round()).abs() > 4 * float((c32 - c64).abs().max())).all())


_DEFORM_REFS = {}


def _deform_refs(n, sources, c, hf, wf, h, w, mode):
    """inputs of test_deform's kinds from the first seed >= 3 whose field keeps every sampling point clear of the texel
    boundaries, and autograd through restate.deform_input in fp64 and in fp32; cached for the two backends"""
    key = (n, sources, c, hf, wf, h, w, mode)
    if key in _DEFORM_REFS:
        return _DEFORM_REFS[key]
    frames = n // sources
    for seed in range(3, 1000):
        g = torch.Generator().manual_seed(seed)
        inp = torch.rand(sources, c, 1, h, w, generator=g)
        field = torch.cat([identity_field(hf, wf).view(1, 1, hf, wf, 2).repeat(n, 1, 1, 1, 1) +
                           0.4 * torch.randn(n, 1, hf, wf, 2, generator=g), torch.zeros(n, 1, hf, wf, 1)], -1)
        dout = torch.randn(n, c, 1, h, w, generator=g, dtype=torch.float64)
        if _clear_of_texel_boundaries(field, h, w, mode):
            break
    else:
        raise AssertionError("no seed below 1000 keeps the sampling points clear of the texel boundaries")
    refs = []
    for dtype in (torch.float64, torch.float32):
        i, f = inp.to(dtype).requires_grad_(True), field.to(dtype).requires_grad_(True)
        out = restate.deform_input(i.repeat_interleave(frames, dim=0) if frames > 1 else i, f,
                                   "nearest" if mode == 0 else "trilinear")
        out.backward(dout.to(dtype))
        refs.append((out.detach()[:, :, 0], i.grad[:, :, 0], f.grad[:, 0, :, :, :2]))
    _DEFORM_REFS[key] = (inp, field, dout, refs[0], refs[1])
    return _DEFORM_REFS[key]


def _deform_case(be, label, frames, sources, c, fsize, msize, mode):
    """the body of test_kernels_motion.test_deform: output at a channel offset with zero pad channels around it, d input
    WRITTEN over NaN with zero pad channels; frames > 1: the _shared_ entries (one source image per `frames` field rows)"""
    (hf, wf), (h, w) = fsize, msize
    n = frames * sources
    inp, field, dout, (o64, di64, df64), (o32, di32, df32) = _deform_refs(n, sources, c, hf, wf, h, w, mode)
    ld = ceil4(c)
    X = be.t(to_nhwc(inp[:, :, 0]))
    FL = be.t(field[:, 0, :, :, :2])
    ldo, off = ld + 8, 3
    OUT = be.zeros(n, h, w, ldo)
    sfx, tail = ("_shared", (n, frames)) if frames > 1 else ("", (n,))
    be.call("mnk_deform%s_fwd" % sfx, X, ld, c, h, w, FL, hf, wf, mode, OUT, ldo, off, *tail)
    DO = be.zeros(n, h, w, ldo)
    DO[..., off:off + c] = be.t(dout[:, :, 0].float().permute(0, 2, 3, 1))
    DI, DF = be.empty(sources, h, w, ld), be.zeros(n, hf, wf, 2)
    DI.fill_(float("nan"))                     # d input is WRITTEN by the gather pass (pad channels 0): no zero fill
    nws = be.query("mnk_deform_bwd_workspace_floats", c, h, w, n)
    be.call("mnk_deform%s_bwd" % sfx, X, ld, c, h, w, FL, hf, wf, mode, DO, ldo, off, DI, DF, *tail, be.empty(nws), nws)
    be.sync()
    out, di, df = OUT.cpu(), DI.cpu(), DF.cpu()
    label = "%s mode %d [%s] " % (label, mode, be.kind)
    assert torch.all(di[..., c:] == 0)
    assert within(label + "out", maxerr, out[..., off:off + c].permute(0, 3, 1, 2), o64, o32, DEFORM_BOUND)[0]
    assert torch.all(out[..., :off] == 0) and torch.all(out[..., off + c:] == 0)
    assert within(label + "dinp", relerr, from_nhwc(di, c), di64, di32, DEFORM_BOUND)[0]
    assert within(label + "dfield", relerr, df, df64, df32, DEFORM_BOUND)[0]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fsize,msize", POOL, ids=POOL_IDS)
def test_deform_off_grid(be, fsize, msize, mode):
    """mnk_deform_fwd / _bwd with the pool's field and map sizes, nearest and bilinear field resize"""
    _deform_case(be, "deform %s" % POOL_IDS[POOL.index((fsize, msize))], 1, 2, 5, fsize, msize, mode)


@pytest.mark.parametrize("mode", [0, 1])
def test_deform_shared_off_grid(be, mode):
    """mnk_deform_shared_fwd / _bwd, three frames per source image, at a float-vs-rational pair"""
    _deform_case(be, "deform-shared 26x14-to-22x46", 3, 2, 5, (26, 14), (22, 46), mode)


# ---- 3. all warps in one launch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want", ["all", "no-dfield", "no-demb"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("table", list(WARP_TABLES_RATIOS))
def test_warp_levels_off_grid(be, table, mode, want):
    """test_kernels_motion.test_warp_levels_direct with hf != wf, He != We and the level sizes of _warp_levels.WARP_TABLES_RATIOS"""
    run_warp_levels(be, table, mode, want)


@pytest.mark.parametrize("mode", [0, 1])
def test_warp_levels_shared_off_grid(be, mode):
    """mnk_warp_levels_shared_fwd / _bwd: three frames of one source image through the float-index table"""
    run_warp_levels(be, "float-index", mode, "all", frames=3)


# ---- 4. the layout kernels' second grid-stride pass -----------------------------------------------------------------------------
CAP = 2048 * 256              # threads of one pass (grid_for caps the grid at 2048 blocks; 8192 for concat2)
SIDE = 728                    # 728 * 728 = 529 984 > CAP


def test_second_pass_ncdhw_to_nhwc_and_back(be):
    """B = C = D = 1 and a 728 x 728 frame: one thread per pixel, 5 696 pixels in the second pass; ld = 2 (a pad channel)"""
    assert CAP < SIDE * SIDE < 2 * CAP
    g = torch.Generator().manual_seed(4)
    x = torch.rand(1, 1, 1, SIDE, SIDE, generator=g)
    out = be.empty(1, SIDE, SIDE, 2)
    be.call("mnk_ncdhw_to_nhwc", be.t(x), out, 1, 1, 1, SIDE, SIDE, 1, 2)
    back = be.empty(1, 1, 1, SIDE, SIDE)
    be.call("mnk_nhwc_to_ncdhw", out, 2, back, 1, 1, 1, SIDE, SIDE)
    be.sync()
    o = out.cpu()
    assert torch.equal(o[..., 0], x[0, 0]) and torch.all(o[..., 1] == 0)
    assert torch.equal(back.cpu(), x)


def test_second_pass_nhwc_to_ncdhw_strided(be):
    """one thread per element of the full-size gradient (728 x 728), step 2: the rows of a 364 x 364 act on the even grid"""
    g = torch.Generator().manual_seed(4)
    ho = SIDE // 2
    a = torch.rand(1, ho, ho, 2, generator=g)
    out = be.empty(1, 1, 1, SIDE, SIDE)
    be.call("mnk_nhwc_to_ncdhw_strided", be.t(a), 2, out, 1, 1, 1, SIDE, SIDE, 2)
    be.sync()
    want = torch.zeros(1, 1, 1, SIDE, SIDE)
    want[0, 0, 0, ::2, ::2] = a[0, :, :, 0]
    assert torch.equal(out.cpu(), want)


def test_second_pass_copy_channels(be):
    """rows * C = 4 more than one pass; plain and accumulating (one fp32 addition: exact)"""
    g = torch.Generator().manual_seed(4)
    rows, c = CAP // 4 + 1, 4
    a, d = torch.randn(rows, 6, generator=g), torch.randn(rows, 5, generator=g)
    A, D, E = be.t(a), be.t(d), be.t(d)
    be.call("mnk_copy_channels", A, 6, 2, D, 5, 1, c, rows, 0)
    be.call("mnk_copy_channels", A, 6, 2, E, 5, 1, c, rows, 1)
    be.sync()
    assert torch.equal(D.cpu()[:, 1:], a[:, 2:]) and torch.equal(D.cpu()[:, 0], d[:, 0])
    assert torch.equal(E.cpu()[:, 1:], d[:, 1:] + a[:, 2:]) and torch.equal(E.cpu()[:, 0], d[:, 0])


def test_second_pass_sumpool2x2(be):
    """two channel quads per output pixel, 514 x 512 output pixels: 2 048 threads beyond one pass"""
    g = torch.Generator().manual_seed(4)
    hd, wd, c = 514, 512, 5
    assert CAP < hd * wd * 2 < 2 * CAP
    x = torch.randn(1, c, 2 * hd, 2 * wd, generator=g)
    Y = be.empty(1, hd, wd, 8)
    be.call("mnk_sumpool2x2", be.t(to_nhwc(x)), 8, Y, 8, 1, 2 * hd, 2 * wd, c)
    be.sync()
    y = Y.cpu()
    refs = [sum(t[:, :, i::2, j::2] for i in (0, 1) for j in (0, 1)) for t in (x.double(), x)]
    assert within("second-pass sumpool2x2 [%s]" % be.kind, maxerr, from_nhwc(y, c), refs[0], refs[1], RESIZE_BOUND)[0]
    assert torch.all(y[..., c:] == 0)


@pytest.mark.parametrize("kind", ["nearest", "bilinear"])
def test_second_pass_resize(be, kind):
    """forward: a (5, 7) source under a 728 x 728 map, C = 1; backward: a 728 x 728 source under a (200, 9) map"""
    g = torch.Generator().manual_seed(4)
    kw = dict(mode="nearest") if kind == "nearest" else dict(mode="bilinear", align_corners=False)
    label = "second-pass resize-%s [%s] " % (kind, be.kind)
    s = torch.randn(1, 1, 5, 7, generator=g)
    O = be.empty(1, SIDE, SIDE, 1)
    be.call("mnk_resize_" + kind, be.t(to_nhwc(s, ld=1)), 1, 5, 7, O, 1, 0, SIDE, SIDE, 1, 1)
    be.sync()
    r64, r32 = F.interpolate(s.double(), size=(SIDE, SIDE), **kw), F.interpolate(s, size=(SIDE, SIDE), **kw)
    if kind == "nearest":
        assert torch.equal(O.cpu().view(SIDE, SIDE), r32[0, 0])
    else:
        assert within(label + "out", maxerr, O.cpu().view(SIDE, SIDE), r64[0, 0], r32[0, 0], RESIZE_BOUND)[0]
    # one thread per source element: the second pass holds the elements from row 720, column 128 on.  A (200, 9) map puts
    # gradient there (nearest: rows 720 and 724, bilinear: rows 720 ... 726), and every buffer shows a write that is missing:
    # _bwd writes over NaN, _bwd_accumulate and the bilinear _bwd add to a non-zero buffer
    hd, wd = 200, 9
    dd = torch.randn(1, 1, hd, wd, generator=g)
    prev = torch.randn(SIDE, SIDE, generator=g)
    grads = []
    for dtype in (torch.float64, torch.float32):
        sr = torch.zeros(1, 1, SIDE, SIDE, dtype=dtype, requires_grad=True)
        if kind == "nearest":
            r = sr[:, :, restate.nearest_index(SIDE, hd)][:, :, :, restate.nearest_index(SIDE, wd)]
        else:
            r = F.interpolate(sr, size=(hd, wd), **kw)
        r.backward(dd.to(dtype))
        grads.append(sr.grad[0, 0])
    g64, g32 = grads
    assert int((g64.reshape(-1)[CAP:] != 0).sum()) >= wd and int((g64.reshape(-1)[:CAP] != 0).sum()) >= wd
    DD = be.t(to_nhwc(dd, ld=1))
    if kind == "nearest":
        DS, DSA = be.empty(1, SIDE, SIDE, 1), be.t(prev.view(1, SIDE, SIDE, 1))
        be.call("mnk_resize_nearest_bwd", DD, 1, 0, hd, wd, DS, 1, SIDE, SIDE, 1, 1)
        be.call("mnk_resize_nearest_bwd_accumulate", DD, 1, 0, hd, wd, DSA, 1, SIDE, SIDE, 1, 1)
        be.sync()
        assert within(label + "dsrc", maxerr, DS.cpu().view(SIDE, SIDE), g64, g32, RESIZE_BOUND)[0]
        assert within(label + "dsrc-accumulated", maxerr, DSA.cpu().view(SIDE, SIDE), prev.double() + g64, prev + g32,
                      RESIZE_BOUND)[0]
    else:
        DS = be.t(prev.view(1, SIDE, SIDE, 1))
        be.call("mnk_resize_bilinear_bwd", DD, 1, 0, hd, wd, DS, 1, SIDE, SIDE, 1, 1)
        be.sync()
        assert within(label + "dsrc", maxerr, DS.cpu().view(SIDE, SIDE), prev.double() + g64, prev + g32, RESIZE_BOUND)[0]


def test_second_pass_concat2(be):
    """ca = cb = 1 (four columns a row): forward rows * 4 and backward rows * (ld_a + ld_b) just above 8192 * 256"""
    g = torch.Generator().manual_seed(4)
    cap = 8192 * 256
    rows = cap // 4 + 1
    a, b = torch.zeros(1, rows, 1, 4), torch.zeros(1, rows, 1, 4)
    a[..., 0], b[..., 0] = torch.randn(1, rows, 1, generator=g), torch.randn(1, rows, 1, generator=g)
    OUT = be.empty(1, rows, 1, 4)
    be.call("mnk_concat2_fwd", be.t(a), 4, 1, be.t(b), 4, 1, 1, OUT, 4, 1, rows)
    be.sync()
    o = OUT.cpu()
    assert torch.equal(o[..., 0], a[..., 0]) and torch.equal(o[..., 1], b[..., 0]) and torch.all(o[..., 2:] == 0)
    rows = cap // 8 + 1
    go = torch.full((1, rows, 1, 4), float("nan"))
    go[..., :2] = torch.randn(1, rows, 1, 2, generator=g)
    GA, GB = be.empty(1, rows, 1, 4), be.empty(1, rows, 1, 4)
    be.call("mnk_concat2_bwd", be.t(go), 4, 1, 1, 1, GA, 4, GB, 4, 1, rows)
    be.sync()
    ga, gb = GA.cpu(), GB.cpu()
    assert torch.equal(ga[..., 0], go[..., 0]) and torch.all(ga[..., 1:] == 0)
    assert torch.equal(gb[..., 0], go[..., 1]) and torch.all(gb[..., 1:] == 0)


# ---- 5. strided layout copies whose step does not divide the frame --------------------------------------------------------------
STRIDED = [(hw, step) for hw in ((9, 13), (7, 6)) for step in (2, 4) if hw[0] // step and hw[1] // step]


@pytest.mark.parametrize("hw,step", STRIDED)
def test_strided_layout_with_a_step_that_does_not_divide(be, hw, step):
    """mnk_ncdhw_to_nhwc == x[..., ::step, ::step] cut to (H // step, W // step) (F.interpolate's floor of the size), and
    mnk_nhwc_to_ncdhw_strided == its adjoint: the rows and columns behind the last full step get zeros"""
    (H, W), B, C, D = hw, 2, 3, 2
    ho, wo = H // step, W // step
    g = torch.Generator().manual_seed(7)
    x = torch.rand(B, C, D, H, W, generator=g)
    out = be.empty(B * D, ho, wo, 4)
    be.call("mnk_ncdhw_to_nhwc", be.t(x), out, B, C, D, H, W, step, 4)
    x64 = x.double().requires_grad_(True)
    ref = x64[..., ::step, ::step][..., :ho, :wo]
    dy = torch.randn(B, C, D, ho, wo, generator=g)
    ref.backward(dy.double())
    DY = be.t(to_nhwc(dy.permute(0, 2, 1, 3, 4).reshape(B * D, C, ho, wo)))
    DX = be.empty(B, C, D, H, W)
    be.call("mnk_nhwc_to_ncdhw_strided", DY, 4, DX, B, C, D, H, W, step)
    be.sync()
    o = out.cpu()
    assert torch.equal(o[..., :C], ref.detach().float().permute(0, 2, 3, 4, 1).reshape(B * D, ho, wo, C))
    assert torch.all(o[..., C:] == 0)
    assert torch.equal(DX.cpu().double(), x64.grad)


def test_strided_layout_refuses_a_step_beyond_the_frame(be):
    """H / step == 0 or W / step == 0: MNK_EINVAL from both entries, nothing written"""
    from mnk._lib import MnkError
    for H, W in ((3, 9), (9, 3)):
        x, out = be.zeros(1, 1, 1, H, W), be.empty(1, 4, 4, 4)
        with pytest.raises(MnkError):
            be.call("mnk_ncdhw_to_nhwc", x, out, 1, 1, 1, H, W, 4, 4)
        with pytest.raises(MnkError):
            be.call("mnk_nhwc_to_ncdhw_strided", out, 4, x, 1, 1, 1, H, W, 4)
        be.sync()
        assert torch.isnan(out.cpu()).all() and torch.all(x.cpu() == 0)
