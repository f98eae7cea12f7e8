"""Several driving frames per source image in the warp kernels (mnk_deform_shared_* / mnk_warp_levels_shared_*,
generator.py:51-58,60-78): field, output and gradient rows v*frames + f read source image v, which exists once.

a. the shared entries equal the plain entries run on the source repeated `frames` times (outputs, field and embedding gradients
   to the bit: the same arithmetic per pixel), and d input -- one image per video, the sum over its frames -- matches the fp64
   autograd of oracle.restate.deform_input on the repeated source;
b. that sum has a fixed order (frame-major, then pixel order): the same bits on every run and an fp32 restatement of the loop;
c. frames = 1 through the shared entries is the plain entries bit for bit;
d. N % frames != 0 is refused before anything is launched, and the workspace queries (with N = field rows) are honest."""
import numpy as np
import pytest
import torch

from _util import to_nhwc, from_nhwc, ceil4, relerr, maxerr
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from oracle import restate

WARP_LEVEL = np.dtype([("inp", "<u8"), ("out", "<u8"), ("dout", "<u8"), ("dinp", "<u8"), ("ld_in", "<i4"), ("C", "<i4"),
                       ("h", "<i4"), ("w", "<i4"), ("ld_out", "<i4"), ("ke", "<i4"), ("emb_off", "<i4"), ("reserved", "<i4")])

# frames, sources, C, (h, w), mode
SHARED_CASES = [
    ("ragged-quad", 3, 2, 5, (16, 16), 0),
    ("trilinear", 3, 2, 6, (8, 8), 1),
    ("scan-rounds", 5, 1, 4, (16, 16), 0),       # frames*P = 1280: a full 1024-point scan round of four frames + a ragged round
    ("straddle", 3, 1, 4, (40, 24), 0),          # P = 960: frames straddle the scan rounds
    ("wide", 3, 2, 300, (4, 4), 0),              # channel slices (pass A) and quad slices (pass B)
    ("one-texel", 2, 2, 7, (1, 1), 0),
]


def _field_size(h):
    return (16, 16) if h != 40 else (20, 12)


def _case_inputs(frames, sources, c, hw, seed=3):
    g = torch.Generator().manual_seed(seed)
    h, w = hw
    hf, wf = _field_size(h)
    n = frames * sources
    src = torch.rand(sources, c, 1, h, w, generator=g)
    field = torch.cat([restate.make_coordinate_grid(hf, wf).view(1, 1, hf, wf, 2).repeat(n, 1, 1, 1, 1) +
                       0.4 * torch.randn(n, 1, hf, wf, 2, generator=g), torch.zeros(n, 1, hf, wf, 1)], -1)
    dout = torch.randn(n, c, 1, h, w, generator=g, dtype=torch.float64)
    return src, field, dout


_REFS = {}


def _reference(tag, frames, sources, c, hw, mode):
    """fp64: deform_input of the repeated source and the gradient of the UN-repeated source (autograd sums the repeats)"""
    if tag not in _REFS:
        src, field, dout = _case_inputs(frames, sources, c, hw)
        s64 = src.double().requires_grad_(True)
        out = restate.deform_input(s64.repeat_interleave(frames, dim=0), field.double(), "nearest" if mode == 0 else "trilinear")
        out.backward(dout)
        _REFS[tag] = (out.detach(), s64.grad.detach())
    return _REFS[tag]


def _same(a, b, mode):
    """bit for bit; under the bilinear field resize the compiler may contract the blends differently (test_kernels_motion)"""
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if mode == 0 else maxerr(a, b) < 1e-6


@pytest.mark.parametrize("tag,frames,sources,c,hw,mode", SHARED_CASES, ids=[t[0] for t in SHARED_CASES])
def test_shared_source_equals_the_repeated_source_per_level(be, tag, frames, sources, c, hw, mode):
    src, field, dout = _case_inputs(frames, sources, c, hw)
    ref_out, ref_dsrc = _reference(tag, frames, sources, c, hw, mode)
    h, w = hw
    hf, wf = _field_size(h)
    n, ld = frames * sources, ceil4(c)
    ldo, off = ld + 8, 3
    X = be.t(to_nhwc(src[:, :, 0]))
    XR = be.t(to_nhwc(src[:, :, 0]).repeat_interleave(frames, dim=0))
    FL = be.t(field[:, 0, :, :, :2])
    DO = be.zeros(n, h, w, ldo)
    DO[..., off:off + c] = be.t(dout[:, :, 0].float().permute(0, 2, 3, 1))
    OUT, OUTR = be.zeros(n, h, w, ldo), be.zeros(n, h, w, ldo)
    be.call("mnk_deform_shared_fwd", X, ld, c, h, w, FL, hf, wf, mode, OUT, ldo, off, n, frames)
    be.call("mnk_deform_fwd", XR, ld, c, h, w, FL, hf, wf, mode, OUTR, ldo, off, n)
    nws = be.query("mnk_deform_bwd_workspace_floats", c, h, w, n)          # N = the field's rows, for both forms
    DI, DF = be.empty(sources, h, w, ld), be.zeros(n, hf, wf, 2)
    DI.fill_(float("nan"))                                                  # d input is WRITTEN (pad channels 0)
    be.call("mnk_deform_shared_bwd", X, ld, c, h, w, FL, hf, wf, mode, DO, ldo, off, DI, DF, n, frames, be.empty(nws), nws)
    DIR, DFR = be.empty(n, h, w, ld), be.zeros(n, hf, wf, 2)
    be.call("mnk_deform_bwd", XR, ld, c, h, w, FL, hf, wf, mode, DO, ldo, off, DIR, DFR, n, be.empty(nws), nws)
    be.sync()
    assert _same(OUT.cpu(), OUTR.cpu(), mode)
    assert _same(DF.cpu(), DFR.cpu(), mode)
    assert maxerr(OUT.cpu()[..., off:off + c].permute(0, 3, 1, 2), ref_out[:, :, 0]) < 1e-5
    di = DI.cpu()
    assert torch.all(di[..., c:] == 0)
    err = relerr(from_nhwc(di, c), ref_dsrc[:, :, 0])
    print("%s: relerr(dinp, fp64 autograd over the repeats) = %.3e" % (tag, err))
    assert err < 1e-5
    # the repeated form's per-copy gradients add up to the same image (another order of the same terms)
    assert relerr(di, DIR.cpu().view(sources, frames, h, w, ld).double().sum(1)) < 1e-5


@pytest.mark.parametrize("tag,frames,sources,c,hw,mode", SHARED_CASES, ids=[t[0] for t in SHARED_CASES])
def test_shared_source_equals_the_repeated_source_all_levels(be, tag, frames, sources, c, hw, mode):
    """mnk_warp_levels_shared_*: the case's level with the key-point embedding behind it, and a second, plain 8 x 8 level"""
    src, field, dout = _case_inputs(frames, sources, c, hw)
    _, ref_dsrc = _reference(tag, frames, sources, c, hw, mode)
    g = torch.Generator().manual_seed(17)
    h, w = hw
    hf, wf = _field_size(h)
    n, ke, he = frames * sources, 6, 8
    shapes = [(c, h, w, ke), (3, 8, 8, 0)]
    srcs = [to_nhwc(src[:, :, 0]), to_nhwc(torch.rand(sources, 3, 8, 8, generator=g))]
    d0 = torch.zeros(n, h, w, ceil4(c + ke))
    d0[..., :c] = dout[:, :, 0].float().permute(0, 2, 3, 1)
    d0[..., c:c + ke] = torch.randn(n, h, w, ke, generator=g)
    douts = [d0, to_nhwc(torch.randn(n, 3, 8, 8, generator=g))]
    emb = torch.randn(n, he, he, ceil4(ke), generator=g)
    emb[..., ke:] = 0
    FL, EMB = be.t(field[:, 0, :, :, :2]), be.t(emb)
    DOS = [be.t(d) for d in douts]

    def run(shared):
        xs = [be.t(s if shared else s.repeat_interleave(frames, dim=0)) for s in srcs]
        outs = [be.empty(n, hh, ww, ceil4(cc + kk)) for cc, hh, ww, kk in shapes]
        dis = [be.empty(*x.shape) for x in xs]
        lv = np.zeros(len(shapes), dtype=WARP_LEVEL)
        for i, (cc, hh, ww, kk) in enumerate(shapes):
            lv[i] = (xs[i].data_ptr(), outs[i].data_ptr(), DOS[i].data_ptr(), dis[i].data_ptr(), xs[i].shape[-1], cc, hh, ww,
                     outs[i].shape[-1], kk, cc, 0)
        tail = (n, frames) if shared else (n,)
        sfx = "_shared" if shared else ""
        # (the level table is a host pointer: the per-call guard check does not see its buffers -- check_all below does)
        be.call("mnk_warp_levels%s_fwd" % sfx, lv.ctypes.data, len(shapes), FL, hf, wf, mode, EMB, emb.shape[-1], he, he, *tail)
        nws = be.query("mnk_warp_levels_bwd_workspace_floats", lv.ctypes.data, len(shapes), n)
        DF, DE = be.empty(n, hf, wf, 2), be.empty(*emb.shape)
        be.call("mnk_warp_levels%s_bwd" % sfx, lv.ctypes.data, len(shapes), FL, hf, wf, mode, DF, DE, emb.shape[-1], he, he, *tail,
                be.empty(nws), nws)
        be.sync()
        be.check_all("after the %s launches" % (sfx or "plain"))
        return [o.cpu() for o in outs], DF.cpu(), DE.cpu(), [d.cpu() for d in dis]

    o1, df1, de1, di1 = run(True)
    o0, df0, de0, di0 = run(False)
    for a, b in zip(o1, o0):
        assert _same(a, b, mode)
    assert _same(df1, df0, mode) and _same(de1, de0, mode)
    for a, b, (cc, hh, ww, _) in zip(di1, di0, shapes):
        assert a.shape[0] == sources and torch.all(a[..., cc:] == 0)
        assert relerr(a, b.view(sources, frames, hh, ww, -1).double().sum(1)) < 1e-5
    assert relerr(from_nhwc(di1[0], c), ref_dsrc[:, :, 0]) < 1e-5


def _loop_restatement(field, dout, sources, frames, c, h, w, hf, wf, fused):
    """fp32, the kernels' own sampling arithmetic: per source image, its frames in order, each frame's pixels in order.
    fused: every step is ONE rounding, acc = fl32(dout * weight + acc), as a fused multiply-add does it (formed in fp64: the
    product of two fp32 numbers is exact there); else the product is rounded to fp32 before it is added."""
    n = sources * frames
    fl = restate.resize_field(torch.cat([field, torch.zeros(n, hf, wf, 1)], -1).view(n, 1, hf, wf, 3), (h, w),
                              "nearest")[:, 0, :, :, :2].float()
    want = torch.zeros(sources, h, w, ceil4(c))
    for b in range(n):
        ix = ((fl[b, ..., 0] + 1.0) / 2.0) * float(w - 1)
        iy = ((fl[b, ..., 1] + 1.0) / 2.0) * float(h - 1)
        fx, fy = torch.floor(ix), torch.floor(iy)
        for py in range(h):
            for px in range(w):
                x0, y0 = int(fx[py, px]), int(fy[py, px])
                for dy in (0, 1):
                    for dx in (0, 1):
                        yy, xx = y0 + dy, x0 + dx
                        if 0 <= yy < h and 0 <= xx < w:
                            wx = (ix[py, px] - fx[py, px]) if dx else ((fx[py, px] + 1.0) - ix[py, px])
                            wy = (iy[py, px] - fy[py, px]) if dy else ((fy[py, px] + 1.0) - iy[py, px])
                            acc = want[b // frames, yy, xx, :c]
                            if fused:
                                want[b // frames, yy, xx, :c] = (dout[b, py, px, :c].double() * (wx * wy).double()
                                                                 + acc.double()).float()
                            else:
                                want[b // frames, yy, xx, :c] = acc + dout[b, py, px, :c] * (wx * wy)
    return want


@pytest.mark.parametrize("kind", ["collapse", "stripes", "random"])
def test_shared_backward_is_deterministic_and_frame_major(be, kind):
    """the field kinds of test_deform_backward_is_deterministic_and_order_exact at 2 sources x 3 frames: many pixels of SEVERAL
    frames land on one source texel.  Three runs give the same bits, and d input equals the frame-major, pixel-ordered fp32 loop
    within the bound of the existing test.  With up to 768 terms on one texel the rounding of each step matters: the gfx950
    build adds every term with a fused multiply-add (v_pk_fma_f32 / v_fmac_f32 in the gather kernel's code), the emulator build
    is plain x86-64 code without one, so the loop is restated with the step of the build under test.  (Measured on the MI355X
    against the unfused loop, `collapse`: 5.2e-6 at a bound of 5.1e-6 -- two chains of 768 differently rounded additions.)"""
    g = torch.Generator().manual_seed(11)
    sources, frames, c, h, w, hf, wf = 2, 3, 5, 16, 16, 16, 16
    n = sources * frames
    grid = restate.make_coordinate_grid(hf, wf).view(1, hf, wf, 2).repeat(n, 1, 1, 1)
    if kind == "collapse":
        field = torch.zeros(n, hf, wf, 2) + 0.13 + 1e-3 * torch.randn(n, hf, wf, 2, generator=g)
    elif kind == "stripes":
        field = grid.clone()
        field[..., 1] = -0.31
    else:
        field = grid + 0.5 * torch.randn(n, hf, wf, 2, generator=g)
    inp = torch.rand(sources, h, w, ceil4(c), generator=g)
    inp[..., c:] = 0
    ld, ldo = ceil4(c), ceil4(c) + 4
    dout = torch.randn(n, h, w, ldo, generator=g)
    X, FL, DO = be.t(inp), be.t(field), be.t(dout)
    nws = be.query("mnk_deform_bwd_workspace_floats", c, h, w, n)
    runs = []
    for _ in range(3):
        DI, DF, WS = be.empty(sources, h, w, ld), be.zeros(n, hf, wf, 2), be.empty(nws)
        DI.fill_(float("nan"))
        be.call("mnk_deform_shared_bwd", X, ld, c, h, w, FL, hf, wf, 0, DO, ldo, 0, DI, DF, n, frames, WS, nws)
        be.sync()
        runs.append((DI.cpu(), DF.cpu()))
    for di, df in runs[1:]:
        assert torch.equal(di.view(torch.int32), runs[0][0].view(torch.int32))
        assert torch.equal(df.view(torch.int32), runs[0][1].view(torch.int32))
    want = _loop_restatement(field, dout, sources, frames, c, h, w, hf, wf, fused=be.kind == "hip")
    other = _loop_restatement(field, dout, sources, frames, c, h, w, hf, wf, fused=be.kind != "hip")
    err = maxerr(runs[0][0], want)
    print("%s: max |dinp - loop| = %.3e (max |want| %.3e); against the loop with the other build's step %.3e" % (
        kind, err, float(want.abs().max()), maxerr(runs[0][0], other)))
    assert err <= 4e-7 * float(want.abs().max() + 1)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("emb_ch", [0, 6, 8])
def test_one_frame_through_the_shared_entries_is_the_plain_entries(be, emb_ch, mode):
    """frames = 1 (the shapes of test_all_warps_in_one_launch_equal_the_per_level_launches): forward, d input, d field and
    d embedding of the shared entries equal the plain entries bit for bit -- they are the same code."""
    g = torch.Generator().manual_seed(6)
    n, hf, wf, he = 2, 16, 16, 8
    field = (torch.rand(n, hf, wf, 2, generator=g) * 2.4 - 1.2)
    lde = ceil4(emb_ch)
    emb = torch.randn(n, he, he, lde, generator=g) if emb_ch else None
    if emb is not None:
        emb[..., emb_ch:] = 0
    shapes = [(8, 4, 4), (5, 8, 8), (4, 16, 16), (3, 32, 32)]
    kes = [emb_ch if i % 2 == 0 else 0 for i in range(len(shapes))]
    inps = [torch.randn(n, h, w, ceil4(c), generator=g) for c, h, w in shapes]
    for t, (c, _, _) in zip(inps, shapes):
        t[..., c:] = 0
    douts = [torch.randn(n, h, w, ceil4(c + ke), generator=g) for (c, h, w), ke in zip(shapes, kes)]
    for d, (c, _, _), ke in zip(douts, shapes, kes):
        d[..., c + ke:] = 0
    FL, EMB = be.t(field), (be.t(emb) if emb is not None else None)
    XS, DOS = [be.t(t) for t in inps], [be.t(d) for d in douts]

    def levels(shared):
        outs = [be.empty(*d.shape) for d in douts]
        dis = [be.empty(*x.shape) for x in inps]
        lv = np.zeros(len(shapes), dtype=WARP_LEVEL)
        for i, ((c, h, w), ke) in enumerate(zip(shapes, kes)):
            lv[i] = (XS[i].data_ptr(), outs[i].data_ptr(), DOS[i].data_ptr(), dis[i].data_ptr(), XS[i].shape[-1], c, h, w,
                     outs[i].shape[-1], ke, c, 0)
        tail, sfx = ((n, 1), "_shared") if shared else ((n,), "")
        be.call("mnk_warp_levels%s_fwd" % sfx, lv.ctypes.data, len(shapes), FL, hf, wf, mode, EMB, lde, he if emb_ch else 0,
                he if emb_ch else 0, *tail)
        nws = be.query("mnk_warp_levels_bwd_workspace_floats", lv.ctypes.data, len(shapes), n)
        DF, DE = be.empty(n, hf, wf, 2), (be.empty(*emb.shape) if emb is not None else None)
        be.call("mnk_warp_levels%s_bwd" % sfx, lv.ctypes.data, len(shapes), FL, hf, wf, mode, DF, DE, lde, he if emb_ch else 0,
                he if emb_ch else 0, *tail, be.empty(nws), nws)
        be.sync()
        be.check_all()
        return [o.cpu() for o in outs] + [d.cpu() for d in dis] + [DF.cpu()] + ([DE.cpu()] if DE is not None else [])

    def per_level(shared):
        res = []
        for (c, h, w), X, DO in zip(shapes, XS, DOS):
            ld, ldo = X.shape[-1], DO.shape[-1]
            OUT, DI, DF = be.zeros(n, h, w, ldo), be.empty(n, h, w, ld), be.zeros(n, hf, wf, 2)
            nws = be.query("mnk_deform_bwd_workspace_floats", c, h, w, n)
            if shared:
                be.call("mnk_deform_shared_fwd", X, ld, c, h, w, FL, hf, wf, mode, OUT, ldo, 0, n, 1)
                be.call("mnk_deform_shared_bwd", X, ld, c, h, w, FL, hf, wf, mode, DO, ldo, 0, DI, DF, n, 1, be.empty(nws), nws)
            else:
                be.call("mnk_deform_fwd", X, ld, c, h, w, FL, hf, wf, mode, OUT, ldo, 0, n)
                be.call("mnk_deform_bwd", X, ld, c, h, w, FL, hf, wf, mode, DO, ldo, 0, DI, DF, n, be.empty(nws), nws)
            be.sync()
            res += [OUT.cpu(), DI.cpu(), DF.cpu()]
        return res

    for form in (levels, per_level):
        new, old = form(True), form(False)
        assert len(new) == len(old)
        for a, b in zip(new, old):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), form.__name__


def test_rows_that_do_not_divide_into_frames_are_refused(be):
    """N % frames != 0: MNK_EINVAL from all four entries, and nothing was launched (every output keeps its fill)"""
    from mnk._lib import MnkError
    g = torch.Generator().manual_seed(2)
    n, frames, c, h, w, hf, wf = 5, 2, 4, 8, 8, 16, 16
    X = be.t(torch.rand(2, h, w, 4, generator=g))
    FL = be.t(torch.rand(n, hf, wf, 2, generator=g) * 2 - 1)
    DO = be.t(torch.randn(n, h, w, 4, generator=g))
    OUT, DI, DF = be.empty(n, h, w, 4), be.empty(2, h, w, 4), be.zeros(n, hf, wf, 2)
    nws = be.query("mnk_deform_bwd_workspace_floats", c, h, w, n)
    lv = np.zeros(1, dtype=WARP_LEVEL)
    lv[0] = (X.data_ptr(), OUT.data_ptr(), DO.data_ptr(), DI.data_ptr(), 4, c, h, w, 4, 0, c, 0)
    nwl = be.query("mnk_warp_levels_bwd_workspace_floats", lv.ctypes.data, 1, n)
    for bad in (2, 0, -1):
        with pytest.raises(MnkError, match="frames"):
            be.call("mnk_deform_shared_fwd", X, 4, c, h, w, FL, hf, wf, 0, OUT, 4, 0, n, bad)
        with pytest.raises(MnkError, match="frames"):
            be.call("mnk_deform_shared_bwd", X, 4, c, h, w, FL, hf, wf, 0, DO, 4, 0, DI, DF, n, bad, be.empty(nws), nws)
        with pytest.raises(MnkError, match="frames"):
            be.call("mnk_warp_levels_shared_fwd", lv.ctypes.data, 1, FL, hf, wf, 0, None, 0, 0, 0, n, bad)
        with pytest.raises(MnkError, match="frames"):
            be.call("mnk_warp_levels_shared_bwd", lv.ctypes.data, 1, FL, hf, wf, 0, DF, None, 0, 0, 0, n, bad, be.empty(nwl), nwl)
    be.sync()
    assert torch.isnan(OUT.cpu()).all() and torch.isnan(DI.cpu()).all() and torch.all(DF.cpu() == 0)


@pytest.mark.parametrize("shrink", [0, 1], ids=["queried-size", "one-float-less"])
def test_shared_backward_workspace_queries_cover_what_the_kernels_write(be, shrink):
    """the plain queries with N = the field's rows are what the shared backward needs: exactly that size runs with intact guards,
    one float less raises (or runs inside the smaller buffer); the C = 300 case uses channel slices, i.e. the most workspace"""
    be.ws_shrink = shrink
    case = SHARED_CASES[4]
    assert case[0] == "wide"
    test_shared_source_equals_the_repeated_source_per_level(be, *case)
    test_shared_source_equals_the_repeated_source_all_levels(be, *case)
    seen = {name: how for name, _, how in be.ws_log}
    assert {"mnk_deform_shared_bwd", "mnk_warp_levels_shared_bwd"} <= set(seen), be.ws_log
    for name in ("mnk_deform_shared_bwd", "mnk_warp_levels_shared_bwd"):
        assert seen[name] == ("exact" if shrink == 0 else "raised"), be.ws_log      # (the query is exact: no float to spare)
