"""Forward convolutions that apply the evaluation-mode norm layer behind them in their own epilogue (include/monkeynet_hip.h:
mnk_conv3x3_fwd_evalnorm, mnk_conv3x3_up_fwd_evalnorm, mnk_conv3x3_evalnorm_form), on guard-banded buffers (tests/_guard.py)
and forced launch plans (force_bm / force_bn / force_splits, as tests/test_kernel_bounds.py):

* equality: z of the fused launch is torch.equal -- equal as floats, bit for bit up to the sign of a zero, pad channels
  included -- to mnk_conv3x3_fwd (mnk_conv3x3_up_fwd) followed by mnk_bn_act_fwd on the same buffers, in fp32 MFMA, with
  MNK_CONV_BF16 and under gemm_bf16x3 / gemm16_bf16x3, at the smallest shapes that reach each way of going wrong;
* the form query: 0 under a split plan and for a pooled position-major shape, where the launch entry refuses; 1 and 2 are what
  then ran (mnk_conv3x3_last_evalnorm_form, mnk_last_plan);
* one fp64 check per form: |z - z64| <= |scale| TAU T + C 2^-24 (|scale| |y64 - mean| + |beta|) per element, averaged over the
  pool window (ReLU and the mean of four are 1-Lipschitz); T = |x| (*) |w| + |bias| and TAU are test_kernel_bounds.py's.

C is what the affine, the ReLU and the pool add to the convolution's own error.  By analysis: (y - mean) rounds once and the fmaf
once, each to half an ulp of at most |scale| |y - mean| + |beta|, and the pool adds three sums of such terms -- one to two
units.  Measured (C_MEASURED): the worst |z - z64(y)| / (2^-24 (|scale| |y - mean| + |beta|)), z64(y) the fp64 affine + ReLU +
mean of four of the fp32 y that the plain launch stores (the fused launch holds the same y in registers: the equality tests).
C = twice the worst of the two backends."""
import pytest
import torch
import torch.nn.functional as F

from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from _util import to_nhwc, from_nhwc, ceil4
import test_kernels_conv as kc
from test_kernel_bounds import TAU, TILES, _tile_ok, _Forced

BF16 = 8                                  # MNK_CONV_BF16
# worst |z - z64(y)| / (2^-24 (|scale| |y - mean| + |beta|)) over the elements of the three fp64 checks in both GEMM modes
# (the pooled form in fp32 MFMA on both; per element 1.78 / 1.78, sub-pixel 1.65 / 1.65, pooled under bf16x3 2.06 / 1.96)
C_MEASURED = {"emu": 2.295, "hip": 2.295}
C = 4.6                                   # twice the worst


def _in_mode(be, name):
    on = 1 if name == "bf16x3" else 0
    try:
        for k in (b"gemm_bf16x3", b"gemm16_bf16x3"):
            be.lib.call("mnk_set_tuning", k, on)
        yield name, (BF16 if name == "bf16-flag" else 0)
    finally:
        for k in (b"gemm_bf16x3", b"gemm16_bf16x3"):
            be.lib.call("mnk_set_tuning", k, 0)


@pytest.fixture(params=["f32-mfma", "bf16-flag", "bf16x3"])
def mode(request, be):
    """-> (name, flags to OR into the launches): fp32 MFMA; the one-pass MNK_CONV_BF16 products; the bf16x3 tuning"""
    yield from _in_mode(be, request.param)


@pytest.fixture(params=["f32-mfma", "bf16x3"])
def accurate_mode(request, be):
    """the two fp32-accurate product forms, which TAU describes (MNK_CONV_BF16 is judged by equality with its own two launches
    here and against fp64 by tests/test_kernels_conv_bf16.py)"""
    yield from _in_mode(be, request.param)


def _norm(cout, seed):
    """coefficients as mnk_bn_eval_coeffs leaves them: any mean, scales of both signs, any beta"""
    g = torch.Generator().manual_seed(100 + seed)
    mean = torch.randn(cout, generator=g) * 0.5
    scale = (torch.rand(cout, generator=g) + 0.5) * torch.where(torch.rand(cout, generator=g) < 0.25, -1.0, 1.0)
    beta = torch.randn(cout, generator=g) * 0.3
    return mean, scale, beta


class _Layer:
    """one convolution (3x3 with an optional up-sampled view, or the sub-pixel form) with its inputs on the backend"""

    def __init__(self, be, n, h, w, c0, c1, cout, ups=0, up=False, clean=True, seed=0):
        # (h, w): the convolution's output size; ups / up: the sources are (h / 2, w / 2)
        self.be, self.geom, self.up, self.ups = be, (n, h, w, c0, c1, cout), up, ups
        case = (n, h, w, c0, c1, cout, 1 if (ups or up) else 0, True, False)
        self.x0, self.x1, self.wt, self.b, _ = kc._inputs(case, seed=seed)
        self.case = case
        self.flags = 0 if up else (int(ups) | (2 if clean else 0))
        padv = 0.0 if (clean or up) else float("nan")
        self.X0 = be.t(to_nhwc(self.x0, pad_value=padv))
        self.X1 = be.t(to_nhwc(self.x1, pad_value=padv)) if self.x1 is not None else None
        self.B = be.t(self.b)
        if up:
            self.wp = be.empty(be.query("mnk_conv3x3_up_packed_floats", cout, c0, c1))
            be.call("mnk_conv3x3_up_pack_fwd", be.t(self.wt), self.wp, cout, c0, c1)
        else:
            self.wp = be.empty(be.query("mnk_conv3x3_packed_floats", cout, c0, c1))
            be.call("mnk_conv3x3_pack_fwd", be.t(self.wt), self.wp, cout, c0, c1)
        self.mean, self.scale, self.beta = _norm(cout, seed)
        self.MEAN, self.SCALE, self.BETA = be.t(self.mean), be.t(self.scale), be.t(self.beta)

    def _src(self):
        return (self.X0, self.X0.shape[-1], self.geom[3], self.X1, self.X1.shape[-1] if self.X1 is not None else 0, self.geom[4])

    def form(self, flags, pool):
        n, h, w, c0, c1, cout = self.geom
        hq, wq = (h // 2, w // 2) if self.up else (h, w)
        return self.be.query("mnk_conv3x3_evalnorm_form", n, hq, wq, c0, c1, cout, self.flags | flags, int(self.up), int(pool))

    def two_launches(self, flags, relu, pool):
        """mnk_conv3x3_fwd / mnk_conv3x3_up_fwd, then mnk_bn_act_fwd -> z (cpu)"""
        be = self.be
        n, h, w, c0, c1, cout = self.geom
        ld = ceil4(cout)
        Y = be.empty(n, h, w, ld)
        if self.up:
            nws = be.query("mnk_conv3x3_up_workspace_floats", n, h // 2, w // 2, c0, c1, cout)
            ws = be.empty(nws) if nws else None
            be.call("mnk_conv3x3_up_fwd", *self._src(), flags, self.wp, self.B, Y, ld, n, h // 2, w // 2, cout, ws, nws, None)
        else:
            nws = be.query("mnk_conv3x3_workspace_floats", n, h, w, c0, c1, cout)
            ws = be.empty(nws) if nws else None
            be.call("mnk_conv3x3_fwd", *self._src(), self.flags | flags, self.wp, self.B, None, 0, Y, ld, n, h, w, cout, ws, nws, None)
        Z = be.empty(n, h // 2 if pool else h, w // 2 if pool else w, ld)
        be.call("mnk_bn_act_fwd", Y, ld, self.MEAN, self.SCALE, self.BETA, Z, ld, 0, n, h, w, cout, int(relu), int(pool))
        be.sync()
        return Z.cpu()

    def plain_y(self, flags):
        """y of the plain launch (cpu)"""
        be = self.be
        n, h, w, c0, c1, cout = self.geom
        Y = be.empty(n, h, w, ceil4(cout))
        if self.up:
            be.call("mnk_conv3x3_up_fwd", *self._src(), flags, self.wp, self.B, Y, Y.shape[-1], n, h // 2, w // 2, cout, None, 0, None)
        else:
            be.call("mnk_conv3x3_fwd", *self._src(), self.flags | flags, self.wp, self.B, None, 0, Y, Y.shape[-1], n, h, w, cout,
                    None, 0, None)
        be.sync()
        return Y.cpu()

    def fused(self, flags, relu, pool):
        be = self.be
        n, h, w, c0, c1, cout = self.geom
        ld = ceil4(cout)
        Z = be.empty(n, h // 2 if pool else h, w // 2 if pool else w, ld)
        norm = (self.MEAN, self.SCALE, self.BETA, int(relu))
        if self.up:
            be.call("mnk_conv3x3_up_fwd_evalnorm", *self._src(), flags, self.wp, self.B, *norm, Z, ld, n, h // 2, w // 2, cout)
        else:
            be.call("mnk_conv3x3_fwd_evalnorm", *self._src(), self.flags | flags, self.wp, self.B, *norm, int(pool), Z, ld, n, h, w, cout)
        be.sync()
        return Z.cpu()

    def check_equal(self, flags, relu, pool, want_form, what):
        """the fused launch against the two launches under the plan in force; the query's answer is what ran"""
        form = self.form(flags, pool)
        assert form == want_form, (what, "form query", form, want_form)
        z = self.fused(flags, relu, pool)
        assert self.be.query("mnk_conv3x3_last_evalnorm_form") == form, (what, "another form ran than the query promised")
        assert kc._last_plan(self.be)[7] == 1, (what, "a fused launch that splits K")
        ref = self.two_launches(flags, relu, pool)
        cout = self.geom[5]
        assert not torch.isnan(z).any(), (what, "unwritten or NaN outputs")
        assert torch.all(z[..., cout:] == 0), (what, "pad channels must be written as zero")
        assert torch.equal(z, ref), (what, "max |diff| = %g at %d elements" % (float((z - ref).abs().max()), int((z != ref).sum())))


# (n, h, w, c0, c1, cout, ups, up, clean): what each exercises
EQ_CASES = [
    ("ragged-M180", (3, 6, 10, 20, 0, 40, 0, False, True)),          # M = 180: ragged against BM 64 and 128, partial last tile
    ("window-is-the-map", (5, 2, 2, 20, 0, 40, 0, False, True)),      # a window is the whole map, a tile spans frames
    ("cout6-rem-lanes", (2, 8, 8, 20, 0, 6, 0, False, True)),         # rem < 4 lanes of the last channel quad
    ("cout33-two-column-tiles", (2, 8, 8, 20, 0, 33, 0, False, True)),
    ("cout13-16wide", (2, 8, 8, 20, 0, 13, 0, False, True)),
    ("cout45-48wide", (2, 8, 8, 20, 0, 45, 0, False, True)),
    ("c0-5-pad-lanes", (2, 8, 8, 5, 0, 20, 0, False, True)),
    ("two-sources-3-4", (2, 8, 8, 3, 4, 20, 0, False, True)),
    ("generic-loader-nan-pads", (2, 8, 8, 5, 0, 20, 0, False, False)),
    ("upsampled-view", (2, 8, 8, 20, 0, 40, 1, False, True)),
    ("sub-pixel", (2, 8, 8, 20, 0, 40, 0, True, True)),
]


def _forms(case, pool):
    """the form a launch of `case` takes under force_splits = 1: none without MNK_CONV_CLEAN_PADS (the generic loader has no such
    kernel); pooled needs the plain 3x3 fast loader"""
    ups, up, clean = case[6:]
    if not clean:
        return 0
    if not pool:
        return 1
    return 2 if (not ups and not up) else 0


@pytest.mark.parametrize("relu", [0, 1], ids=["affine", "relu"])
@pytest.mark.parametrize("tag,case", EQ_CASES, ids=[c[0] for c in EQ_CASES])
def test_fused_launch_equals_the_two_launches(be, mode, tag, case, relu):
    name, flags = mode
    n, h, w, c0, c1, cout, ups, up, clean = case
    layer = _Layer(be, n, h, w, c0, c1, cout, ups, up, clean, seed=len(tag))
    plans = [(0, 0, 1)]
    if tag == "ragged-M180":
        plans = [(64, 64, 1), (128, 64, 1)]
    if tag == "cout33-two-column-tiles":
        plans = [(128, 32, 1), (0, 0, 1)]
    for plan in plans:
        for pool in ((0,) if up else (0, 1)):
            want = _forms(case, pool)
            with _Forced(be, plan):
                if want:
                    layer.check_equal(flags, relu, pool, want, (tag, name, plan, "pool" if pool else "no pool"))
                else:
                    _refused(layer, flags, relu, pool)


def _refused(layer, flags, relu, pool):
    from mnk._lib import MnkError
    assert layer.form(flags, pool) == 0
    with pytest.raises(MnkError, match="evalnorm_form answers 0"):
        layer.fused(flags, relu, pool)


@pytest.mark.parametrize("pool", [0, 1], ids=["no-pool", "pool"])
def test_every_tile_runs_both_forms(be, mode, pool):
    """every block tile the kernels are instantiated for, unsplit, at a ragged M"""
    name, flags = mode
    layers = {}
    for bm, bn in TILES:
        cout = 13 if bn == 16 else 40
        assert _tile_ok(bm, bn, cout, 1)
        if cout not in layers:
            layers[cout] = _Layer(be, 3, 6, 10, 20, 0, cout, seed=bn)
        with _Forced(be, (bm, bn, 1)):
            layers[cout].check_equal(flags, 1, pool, 2 if pool else 1, (name, bm, bn))
            assert kc._last_plan(be)[5:7] == (bm, bn), "the forced tile was not taken"


def test_position_major_launch_fuses_per_element_and_refuses_the_pool(be, mode):
    """a 2x2 map with 128 frames walks position-major under the default ktap_skip_min (fp32 products only): the per-element form
    runs on that row map; the pooled form has no such kernel -- the query answers 0 and the launch refuses.  The one-pass and
    bf16x3 products have no position-major rows: there the pooled form runs."""
    name, flags = mode
    layer = _Layer(be, 128, 2, 2, 20, 0, 70, seed=5)           # (70 channels: a 64-wide 32x32 tile -- the 16x16 tiles have no such rows)
    with _Forced(be, (0, 0, 1)):
        layer.check_equal(flags, 1, 0, 1, (name, "per element"))
        if name == "f32-mfma":
            _refused(layer, flags, 1, 1)
        else:
            layer.check_equal(flags, 1, 1, 2, (name, "pooled, frame-major plan"))


def test_split_plans_are_refused(be, mode):
    name, flags = mode
    layer = _Layer(be, 2, 8, 8, 20, 0, 40, seed=6)
    up = _Layer(be, 2, 8, 8, 20, 0, 40, up=True, seed=7)
    with _Forced(be, (0, 0, 3)):
        for pool in (0, 1):
            _refused(layer, flags, 1, pool)
        _refused(up, flags, 1, 0)
        assert kc._last_plan(be)[7] == 3
    # what these shapes do once nothing is forced is the plan rule's business; forced to one split they fuse
    with _Forced(be, (0, 0, 1)):
        assert layer.form(flags, 0) == 1 and layer.form(flags, 1) == 2 and up.form(flags, 0) == 1


def test_invalid_requests_are_rejected(be):
    from mnk._lib import MnkError
    layer = _Layer(be, 2, 8, 8, 20, 0, 40, seed=8)
    with _Forced(be, (0, 0, 1)):
        assert layer.form(4, 0) == 0 and layer.form(16, 0) == 0           # MNK_CONV_DEFER_SPLITK, MNK_CONV_BF16_TRAIN
        for bad in (4, 16):
            with pytest.raises(MnkError):
                layer.fused(bad, 1, 0)
        odd = _Layer(be, 2, 6, 5, 20, 0, 40, seed=9)                    # odd W: no pool
        assert odd.form(0, 1) == 0 and odd.form(0, 0) == 1
        with pytest.raises(MnkError):
            odd.fused(0, 1, 1)


def _fp64(layer, relu, pool):
    """-> (z64, bound terms): the fp64 convolution + affine + ReLU + mean of four, T = |x| (*) |w| + |bias|, and
    A = |scale| |y64 - mean| + |beta|, both pushed through the pool's average"""
    n, h, w, c0, c1, cout = layer.geom
    y64 = kc._ref_fwd(layer.case, layer.x0, layer.x1, layer.wt, layer.b, None)
    x = layer.x0 if layer.x1 is None else torch.cat([layer.x0, layer.x1], 1)
    if layer.case[6]:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    t = F.conv2d(x.abs().double(), layer.wt.abs().double(), layer.b.abs().double(), padding=1)
    m, s, b = (v.double()[None, :, None, None] for v in (layer.mean, layer.scale, layer.beta))
    z64 = (y64 - m) * s + b
    if relu:
        z64 = z64.clamp_min(0)
    first, second = s.abs() * TAU * t, 2.0 ** -24 * (s.abs() * (y64 - m).abs() + b.abs())
    if pool:
        z64, first, second = (F.avg_pool2d(v, 2) for v in (z64, first, second))
    return z64, first, second


@pytest.mark.parametrize("form", ["per-element", "sub-pixel", "pooled"])
def test_fused_launch_against_fp64(be, accurate_mode, form):
    name, flags = accurate_mode
    up, pool = form == "sub-pixel", form == "pooled"
    layer = _Layer(be, 3, 6, 10, 20, 13, 70, up=up, seed=11) if not up else _Layer(be, 2, 8, 12, 20, 13, 70, up=True, seed=12)
    cout = layer.geom[5]
    with _Forced(be, (0, 0, 1)):
        z = layer.fused(0, 1, pool)
        assert be.query("mnk_conv3x3_last_evalnorm_form") == (2 if pool else 1)
        y = from_nhwc(layer.plain_y(0), cout).double()
    z64, first, second = _fp64(layer, 1, pool)
    err = (from_nhwc(z, cout).double() - z64).abs()
    # the measurement behind C: the affine + ReLU + pool part alone, on the kernel's own fp32 y
    m, s, b = (v.double()[None, :, None, None] for v in (layer.mean, layer.scale, layer.beta))
    zy, ay = ((y - m) * s + b).clamp_min(0), 2.0 ** -24 * (s.abs() * (y - m).abs() + b.abs())
    if pool:
        zy, ay = F.avg_pool2d(zy, 2), F.avg_pool2d(ay, 2)
    need = float(((from_nhwc(z, cout).double() - zy).abs() / ay.clamp_min(1e-30)).max())
    print("evalnorm fp64 %s %s %s: C needed by affine + ReLU + pool = %.3f; worst err / bound = %.3f"
          % (be.kind, name, form, need, float((err / (first + C * second)).max())))
    assert bool((err <= first + C * second).all()), (form, need)
    assert torch.all(z[..., cout:] == 0)
