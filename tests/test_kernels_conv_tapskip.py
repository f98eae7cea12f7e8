"""Position-major rows + block-uniform tap skipping of the forward / data-gradient implicit GEMM (tuning value ktap_skip;
csrc/conv3x3.hip: row_pixel, TapCursor, plan_taps).  Every case runs the same launch with ktap_skip = 1 and 0 under a forced
plan (tile, splits) and asks for: equal outputs (and equal raw split-K partials), the fp64 restatement at the tolerance of
test_kernels_conv.py, and a recorded `executed` figure equal to a count made here from the geometry alone.
The same bodies run on the CPU emulator build (-m "not gpu") and on the MI355X (-m gpu)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import to_nhwc, from_nhwc, ceil4, relerr
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)

TOL = 2e-6          # test_kernels_conv.py: every forward / data-gradient form against fp64


@pytest.fixture(autouse=True)
def every_skippable_launch(be):
    """the plan's pay-off threshold (ktap_skip_min) is a measured value and may move: here every launch that can skip takes the form"""
    v = ctypes.c_int()
    be.lib.call("mnk_get_tuning", b"ktap_skip_min", ctypes.addressof(v))
    be.lib.call("mnk_set_tuning", b"ktap_skip_min", 0)
    yield
    for name in ("force_bm", "force_bn", "force_splits"):
        be.lib.call("mnk_set_tuning", name.encode(), 0)
    be.lib.call("mnk_set_tuning", b"ktap_skip", 1)
    be.lib.call("mnk_set_tuning", b"ktap_skip_min", v.value)


def _last_plan(be):
    out = np.zeros(8, dtype=np.int64)
    be.lib.call("mnk_last_plan", out.ctypes.data)
    return tuple(int(v) for v in out)


def _tile_masks(bm, frames, H, W, Hi, Wi, kh, kw, pad, stride, phases):
    """[(rows, tap mask)] of every M tile of every phase of a position-major launch: GEMM row m = position * frames + frame,
    a tap's bit is set when the tap is inside the (Hi, Wi) source for at least one position of the tile"""
    M = frames * H * W
    out = []
    for phase in range(phases):
        py, px = pad - (phase >> 1), pad - (phase & 1)
        for m0 in range(0, M, bm):
            m1 = min(m0 + bm, M)
            mask = 0
            for p in range(m0 // frames, (m1 - 1) // frames + 1):
                h, w = (p // W) * stride, (p % W) * stride
                for ky in range(kh):
                    for kx in range(kw):
                        if 0 <= h + ky - py < Hi and 0 <= w + kx - px < Wi:
                            mask |= 1 << (ky * kw + kx)
            out.append((m1 - m0, mask))
    return out


def _executed(tiles, cout, cin):
    """what the recorder must report: it is the host plan's count of issued (row, tap) pairs (not a device counter), so this
    pins the accounting; that the kernel skips no MORE than it may is pinned by the equal outputs"""
    return 2.0 * cout * cin * sum(rows * bin(mask).count("1") for rows, mask in tiles)


def _empty_splits(tiles, ntaps, chunks, splits):
    """(tile, split) pairs whose K range [split * per, ...) holds no step of a set tap"""
    ksteps = ntaps * chunks
    per = -(-ksteps // splits)
    n = 0
    for _, mask in tiles:
        for s0 in range(0, ksteps, per):
            n += not any(mask >> (s % ntaps) & 1 for s in range(s0, min(s0 + per, ksteps)))
    return n


def _ab(be, plan, launch, geom, cout, cin, ref, expect_skip=True):
    """launch() -> (y, ws or None, extra or None) with ktap_skip = 0 and 1 under the forced plan; returns what knob 1 left"""
    bm, bn, splits = plan
    for name, v in (("force_bm", bm), ("force_bn", bn), ("force_splits", splits)):
        be.lib.call("mnk_set_tuning", name.encode(), v)
    got = {}
    for knob in (0, 1):
        be.lib.call("mnk_set_tuning", b"ktap_skip", knob)
        be.lib.cdll.mnk_prof_reset()
        be.lib.cdll.mnk_prof_enable(1)
        try:
            y, ws, extra = launch()
            be.sync()
        finally:
            be.lib.cdll.mnk_prof_enable(0)
        ex = ctypes.c_double()
        be.lib.cdll.mnk_prof_query_executed(0, ctypes.byref(ex))          # group 0: conv3x3_igemm
        be.lib.cdll.mnk_prof_reset()
        p = _last_plan(be)
        assert p[5:7] == (bm, bn), ("the forced tile was refused", p)
        got[knob] = (y.cpu(), None if ws is None else ws.cpu(), None if extra is None else extra.cpu(), ex.value, p[7])
    y0, ws0, st0, ex0, sp0 = got[0]
    y1, ws1, st1, ex1, sp1 = got[1]
    assert sp0 == sp1, "the split count must not depend on the knob"
    frames, H, W, Hi, Wi, kh, kw, pad, stride, phases = geom
    full = 2.0 * frames * H * W * phases * kh * kw * cout * cin
    tiles = _tile_masks(bm, *geom)
    want = _executed(tiles, cout, cin) if expect_skip else full
    print("plan", plan, "splits", sp1, "executed", ex0, "->", ex1, "count", want, "full", full,
          "relerr", relerr(from_nhwc(y1, cout), ref))
    assert ex0 == full
    assert ex1 == want
    if expect_skip:
        assert want < full, "the case skips nothing"
    assert torch.equal(y1, y0)
    assert (ws1 is None) == (sp1 == 1)
    if ws1 is not None:
        assert torch.equal(ws1, ws0), "raw split-K partials"
    if st1 is not None:
        assert torch.equal(st1, st0), "column sums"
    assert relerr(from_nhwc(y1, cout), ref) < TOL
    assert torch.all(y1[..., cout:] == 0)
    return tiles, sp1


# ---- the discriminator's 4x4 / pad 0 data gradient: a pad-3 correlation over dy ------------------------------------------------
# (ho, frames, channels of dy, channels of dx, tile); the forced splits are 1, 3 and K steps / 8 (splits of half a chunk: the
# corner tiles' only taps are the last ones of a chunk, so their first half-chunk split holds no step)
D4_CASES = [(2, 64, 16, 16, (64, 64)), (2, 48, 48, 33, (64, 64)), (2, 8, 32, 64, (128, 64)),
            (10, 64, 16, 24, (64, 64)), (10, 48, 16, 64, (64, 128)), (10, 8, 48, 30, (128, 32))]


@pytest.mark.parametrize("splits", [1, 3, "half-chunk"])
@pytest.mark.parametrize("case", D4_CASES)
def test_discriminator_data_gradient(be, case, splits):
    ho, n, cdy, cdx, tile = case
    hi = ho + 3
    chunks = (cdy + 15) // 16
    half_chunk = splits == "half-chunk"
    if half_chunk:
        splits = 2 * chunks
    g = torch.Generator().manual_seed(41)
    dy = torch.randn(n, cdy, ho, ho, generator=g)
    wt = torch.randn(cdy, cdx, 4, 4, generator=g) * 0.2             # forward: cdx -> cdy channels
    ref = F.conv_transpose2d(dy.double(), wt.double())
    DY, ldy, ldx = be.t(to_nhwc(dy)), ceil4(cdy), ceil4(cdx)
    wpd = be.empty(be.query("mnk_conv2d_packed_floats", cdx, cdy, 0, 16))
    be.call("mnk_conv2d_pack_dgrad", be.t(wt), wpd, cdy, cdx, 0, cdx, 16)

    def launch():
        nws = be.query("mnk_conv2d_workspace_floats", n, hi, hi, cdy, 0, cdx, 16)
        ws = be.empty(nws) if nws else None
        DX = be.empty(n, hi, hi, ldx)
        be.call("mnk_conv2d_fwd", DY, ldy, cdy, None, 0, 0, 2, ho, ho, 4, 4, 3, wpd, None, None, 0, DX, ldx, n, hi, hi, cdx,
                ws, nws, None)
        return DX, ws, None

    tiles, sp = _ab(be, tile + (splits,), launch, (n, hi, hi, ho, ho, 4, 4, 3, 1, 1), cdx, cdy, ref)
    if half_chunk:
        assert sp == 2 * chunks, "the forced split count was altered"
        assert _empty_splits(tiles, 16, chunks, sp) > 0, "the case was meant to leave a split without a step"


# ---- 3x3 / pad 1 forward and data gradient on 2x2 and 4x4 maps ----------------------------------------------------------------
# (map, frames, c0, c1, cout, tile, splits, ups); ups: the sources are half the map's size and read through the x2 up-sampled
# view of the 3x3 loader (forward only: the data gradient of such a layer is taken at full resolution and pooled)
S3_CASES = [(2, 64, 20, 13, 40, (64, 64), 1, 0), (2, 32, 48, 0, 18, (64, 64), 3, 0), (4, 64, 20, 13, 64, (64, 128), 3, 0),
            (4, 32, 16, 0, 33, (128, 64), 1, 0), (4, 64, 24, 17, 40, (64, 64), 3, 1), (2, 32, 16, 0, 20, (64, 64), 1, 1)]


@pytest.mark.parametrize("case", S3_CASES)
def test_small_map_forward_and_data_gradient(be, case):
    hw, n, c0, c1, cout, tile, splits, ups = case
    g = torch.Generator().manual_seed(43)
    hs = hw // 2 if ups else hw
    x0 = torch.randn(n, c0, hs, hs, generator=g)
    x1 = torch.randn(n, c1, hs, hs, generator=g) if c1 else None
    wt = torch.randn(cout, c0 + c1, 3, 3, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    res = torch.randn(n, cout, hw, hw, generator=g)
    x = (x0 if x1 is None else torch.cat([x0, x1], 1)).double().requires_grad_(True)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest") if ups else x, wt.double(), b.double(), padding=1)
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy.double())
    W = be.t(wt)
    X0, X1, R, B = be.t(to_nhwc(x0)), be.t(to_nhwc(x1)) if c1 else None, be.t(to_nhwc(res)), be.t(b)
    wp = be.empty(be.query("mnk_conv3x3_packed_floats", cout, c0, c1))
    be.call("mnk_conv3x3_pack_fwd", W, wp, cout, c0, c1)
    ldy = ceil4(cout)

    def fwd():
        nws = be.query("mnk_conv3x3_workspace_floats", n, hw, hw, c0, c1, cout)
        ws = be.empty(nws) if nws else None
        Y = be.empty(n, hw, hw, ldy)
        be.call("mnk_conv3x3_fwd", X0, X0.shape[-1], c0, X1, X1.shape[-1] if c1 else 0, c1, 2 | ups, wp, B, R, ldy, Y, ldy, n, hw, hw,
                cout, ws, nws, None)
        return Y, ws, None

    geom = (n, hw, hw, hw, hw, 3, 3, 1, 1, 1)
    _ab(be, tile + (splits,), fwd, geom, cout, c0 + c1, ref.detach() + res.double())
    if ups:
        return
    DY = be.t(to_nhwc(dy))
    for c_start, c_cnt in ((0, c0),) + (((c0, c1),) if c1 else ()):
        wpd = be.empty(be.query("mnk_conv3x3_packed_floats", c_cnt, cout, 0))
        be.call("mnk_conv3x3_pack_dgrad", W, wpd, cout, c0 + c1, c_start, c_cnt)
        ld = ceil4(c_cnt)

        def dgrad():
            nws = be.query("mnk_conv3x3_workspace_floats", n, hw, hw, cout, 0, c_cnt)
            ws = be.empty(nws) if nws else None
            DX = be.empty(n, hw, hw, ld)
            be.call("mnk_conv3x3_fwd", DY, ldy, cout, None, 0, 0, 2, wpd, None, None, 0, DX, ld, n, hw, hw, c_cnt, ws, nws, None)
            return DX, ws, None

        # (a 128-row tile of the 2x2 map at 32 frames holds all four positions: nothing to skip)
        _ab(be, (128, 32, splits) if c_cnt <= 32 and hw > 2 else (64, 64, splits), dgrad, geom, c_cnt, cout,
            x.grad[:, c_start:c_start + c_cnt])


# ---- sub-pixel forward from 1x1 and 2x2 sources, and the matching data gradient (4x4 / stride 2 over dy) -------------------------
UP_CASES = [(1, 64, 32, 0, 24, (64, 64), 1), (1, 32, 20, 13, 40, (64, 64), 3), (2, 64, 16, 0, 33, (128, 64), 3),
            (2, 32, 40, 0, 64, (64, 128), 1)]


@pytest.mark.parametrize("case", UP_CASES)
def test_subpixel_forward_and_data_gradient(be, case):
    hw, n, c0, c1, cout, tile, splits = case
    g = torch.Generator().manual_seed(47)
    x0 = torch.randn(n, c0, hw, hw, generator=g)
    x1 = torch.randn(n, c1, hw, hw, generator=g) if c1 else None
    wt = torch.randn(cout, c0 + c1, 3, 3, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    x = (x0 if x1 is None else torch.cat([x0, x1], 1)).double().requires_grad_(True)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt.double(), b.double(), padding=1)
    dy = torch.randn(ref.shape, generator=g)
    ref.backward(dy.double())
    W, B = be.t(wt), be.t(b)
    X0, X1 = be.t(to_nhwc(x0)), be.t(to_nhwc(x1)) if c1 else None
    wp = be.empty(be.query("mnk_conv3x3_up_packed_floats", cout, c0, c1))
    be.call("mnk_conv3x3_up_pack_fwd", W, wp, cout, c0, c1)
    ldy = ceil4(cout)

    def fwd():
        nws = be.query("mnk_conv3x3_up_workspace_floats", n, hw, hw, c0, c1, cout)
        ws = be.empty(nws) if nws else None
        Y = be.empty(n, 2 * hw, 2 * hw, ldy)
        be.call("mnk_conv3x3_up_fwd", X0, X0.shape[-1], c0, X1, X1.shape[-1] if c1 else 0, c1, 0, wp, B, Y, ldy, n, hw, hw, cout,
                ws, nws, None)
        return Y, ws, None

    _ab(be, tile + (splits,), fwd, (n, hw, hw, hw, hw, 2, 2, 1, 1, 4), cout, c0 + c1, ref.detach())
    DY = be.t(to_nhwc(dy))
    for c_start, c_cnt in ((0, c0),) + (((c0, c1),) if c1 else ()):
        wd = be.empty(be.query("mnk_conv3x3_up_dgrad_packed_floats", cout, c_cnt))
        be.call("mnk_conv3x3_up_pack_dgrad", W, wd, cout, c0 + c1, c_start, c_cnt)
        ld = ceil4(c_cnt)

        def dgrad():
            nws = be.query("mnk_conv3x3_up_dgrad_workspace_floats", n, hw, hw, cout, c_cnt)
            ws = be.empty(nws) if nws else None
            DX = be.empty(n, hw, hw, ld)
            be.call("mnk_conv3x3_up_dgrad", DY, ldy, cout, wd, DX, ld, n, hw, hw, c_cnt, ws, nws)
            return DX, ws, None

        _ab(be, (128, 32, splits) if c_cnt <= 32 else (64, 64, splits), dgrad, (n, hw, hw, 2 * hw, 2 * hw, 4, 4, 1, 2, 1), c_cnt,
            cout, x.grad[:, c_start:c_start + c_cnt])


# ---- an unsplit launch whose epilogue leaves per-block column sums keeps the frame-major order ---------------------------------
def test_column_sum_launch_keeps_the_frame_major_order(be):
    hw, n, c0, cout = 4, 64, 20, 40
    g = torch.Generator().manual_seed(53)
    x0 = torch.randn(n, c0, hw, hw, generator=g)
    wt = torch.randn(cout, c0, 3, 3, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    ref = F.conv2d(x0.double(), wt.double(), b.double(), padding=1)
    X0, B, ldy = be.t(to_nhwc(x0)), be.t(b), ceil4(cout)
    wp = be.empty(be.query("mnk_conv3x3_packed_floats", cout, c0, 0))
    be.call("mnk_conv3x3_pack_fwd", be.t(wt), wp, cout, c0, 0)

    def fwd():
        assert be.query("mnk_conv3x3_workspace_floats", n, hw, hw, c0, 0, cout) == 0
        nst = be.query("mnk_conv3x3_stats_floats", n, hw, hw, c0, 0, cout)
        st = be.empty(nst)
        Y = be.empty(n, hw, hw, ldy)
        be.call("mnk_conv3x3_fwd", X0, X0.shape[-1], c0, None, 0, 0, 2, wp, B, None, 0, Y, ldy, n, hw, hw, cout, None, 0, st)
        return Y, None, st

    _ab(be, (64, 64, 1), fwd, (n, hw, hw, hw, hw, 3, 3, 1, 1, 1), cout, c0, ref, expect_skip=False)
