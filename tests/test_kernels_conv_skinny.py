"""Weight-streaming ("skinny") 3x3 convolutions for batch-1 evaluation (include/monkeynet_hip.h: mnk_conv3x3_skinny_pack,
mnk_conv3x3_skinny_form / _splits / _workspace_floats, mnk_conv3x3_skinny_fwd), on guard-banded buffers (tests/_guard.py):

* fp64 bound: the split partials of the skinny launch, summed by mnk_bn_eval_split_fwd with identity norm coefficients and no
  ReLU, obey |y - y64| <= TAU T per element, T = |x| (*) |w| + |bias| and TAU test_kernel_bounds.py's -- any fixed fp32 summation
  order meets it at these K.  With MNK_CONV_BF16 the reference is the fp64 convolution of the operands rounded to bf16 on the
  host and T is made of the rounded operands: the products are exact, so the bound and TAU are the same;
* the same through the full norm epilogue (scales of both signs, ReLU, pool) with the per-element bound and the constant C of
  tests/test_kernels_conv_evalnorm.py; pad channels of z are zero;
* two runs are bit-equal; the bf16 pack computes what the fp32 pack of host-rounded operands computes, bit for bit;
* the form query at skinny_rows and skinny_rows + 1, the refused launch (MNK_EINVAL, a NaN-filled workspace untouched),
  mnk_last_plan and the workspace query.

Every case runs under force_splits 1, 2 and 5, in fp32 and in bf16."""
import pytest
import torch
import torch.nn.functional as F

from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from _util import to_nhwc, from_nhwc, ceil4
import test_kernels_conv as kc
from test_kernel_bounds import TAU, _Forced
from test_kernels_conv_evalnorm import C, _norm

UPS, BF16 = 1, 8                          # MNK_CONV_UPSAMPLED, MNK_CONV_BF16
ROWS = 64                                 # skinny_rows for the value tests: the largest the kernel must accept

# (tag, (n, h, w of the OUTPUT, c0, c1, cout), up-sampled, pooled)
CASES = [
    # every row touches padding, Cout no multiple of 4 or 16; K = 9 * 33 = 297 does not divide by 5
    ("all-padding-two-sources", (1, 2, 2, 20, 13, 45), 0, 0),
    ("plain-one-source", (1, 4, 4, 36, 0, 70), 0, 0),
    ("two-images-halo", (2, 2, 2, 20, 0, 40), 0, 0),            # the halo must not read across images
    ("r12-partial-row-tile", (3, 2, 2, 8, 5, 10), 0, 0),        # R = 12, Cout smaller than a tile
    ("up-from-1x1", (1, 2, 2, 24, 9, 40), 1, 0),
    ("up-from-2x2", (1, 4, 4, 20, 13, 45), 1, 0),
    ("up-from-3x2", (1, 6, 4, 16, 0, 33), 1, 0),                # non-square, R = 24, K = 9 * 16
    ("pooled-4x4", (1, 4, 4, 36, 0, 70), 0, 1),
    ("pooled-2x2", (1, 2, 2, 20, 13, 45), 0, 1),
]
SPLITS = (1, 2, 5)


def _bf16(v):
    return v.to(torch.bfloat16).to(torch.float32)


_DEFAULTS = {}
_KNOBS = (b"skinny_rows", b"skinny_up_min_weights")


@pytest.fixture
def rows64(be, _remember_default):
    """every case is taken: 64 rows, and no up-sampled layer is left to the sub-pixel launch for its short weight stream"""
    be.lib.call("mnk_set_tuning", b"skinny_rows", ROWS)
    be.lib.call("mnk_set_tuning", b"skinny_up_min_weights", 0)
    return be


@pytest.fixture(autouse=True)
def _remember_default(be):
    """the library's own values, read before any test changes them, are what every test puts back"""
    import ctypes
    if be.kind not in _DEFAULTS:
        vals = []
        for k in _KNOBS:
            v = ctypes.c_int(0)
            be.lib.cdll.mnk_get_tuning(k, ctypes.byref(v))
            vals.append(v.value)
        _DEFAULTS[be.kind] = vals
    yield
    for k, v in zip(_KNOBS, _DEFAULTS[be.kind]):
        be.lib.call("mnk_set_tuning", k, v)


class _Skinny:
    """one layer: inputs on the backend, both packs, the skinny launch and the second stage"""

    def __init__(self, be, geom, ups, seed, prerounded=False):
        self.be, self.geom, self.ups = be, geom, ups
        n, h, w, c0, c1, cout = geom
        self.case = (n, h, w, c0, c1, cout, ups, True, False)
        x0, x1, wt, b, _ = kc._inputs(self.case, seed=seed)
        if prerounded:
            x0, x1, wt = _bf16(x0), (_bf16(x1) if x1 is not None else None), _bf16(wt)
        self.x0, self.x1, self.wt, self.b = x0, x1, wt, b
        self.X0 = be.t(to_nhwc(x0, pad_value=float("nan")))          # pad channels are never read
        self.X1 = be.t(to_nhwc(x1, pad_value=float("nan"))) if x1 is not None else None
        self.B = be.t(b)
        self.packs = {}
        W = be.t(wt)
        for bf in (0, 1):
            nf = be.query("mnk_conv3x3_skinny_packed_floats", cout, c0, c1, bf)
            assert nf > 0
            self.packs[bf] = be.empty(nf)
            be.call("mnk_conv3x3_skinny_pack", W, self.packs[bf], cout, c0, c1, bf)
        assert be.query("mnk_conv3x3_skinny_packed_floats", cout, c0, c1, 1) * 2 == be.query(
            "mnk_conv3x3_skinny_packed_floats", cout, c0, c1, 0)

    def _src(self):
        c0, c1 = self.geom[3:5]
        return (self.X0, self.X0.shape[-1], c0, self.X1, self.X1.shape[-1] if self.X1 is not None else 0, c1)

    def partials(self, flags, pack=None):
        """-> (ws on the backend, splits): the skinny launch alone"""
        be = self.be
        n, h, w, c0, c1, cout = self.geom
        flags |= self.ups
        splits = be.query("mnk_conv3x3_skinny_splits", n, h, w, c0, c1, cout)
        nws = be.query("mnk_conv3x3_skinny_workspace_floats", n, h, w, c0, c1, cout)
        assert nws == splits * n * h * w * ceil4(cout), "the workspace query is splits x R x ldw"
        ws = be.empty(nws)
        wp = self.packs[1 if flags & BF16 else 0] if pack is None else pack
        be.call("mnk_conv3x3_skinny_fwd", *self._src(), flags, wp, n, h, w, cout, ws, nws)
        be.sync()
        return ws, splits

    def second_stage(self, ws, splits, mean, scale, beta, relu, pool, bias=True):
        be = self.be
        n, h, w, c0, c1, cout = self.geom
        ld = ceil4(cout)
        Z = be.empty(n, h // 2 if pool else h, w // 2 if pool else w, ld)
        be.call("mnk_bn_eval_split_fwd", ws, splits, ld, 1, self.B if bias else None, be.t(mean), be.t(scale), be.t(beta), Z, ld, n, h,
                w, cout, int(relu), int(pool))
        be.sync()
        return Z.cpu()

    def y(self, flags, pack=None):
        """the convolution's output: the partials summed with identity norm coefficients and no ReLU"""
        cout = self.geom[5]
        ws, splits = self.partials(flags, pack)
        return self.second_stage(ws, splits, torch.zeros(cout), torch.ones(cout), torch.zeros(cout), 0, 0)

    def fp64(self, bf16):
        """-> (y64, T) of the operands (rounded to bf16 on the host when `bf16`)"""
        x0, x1, wt = self.x0, self.x1, self.wt
        if bf16:
            x0, x1, wt = _bf16(x0), (_bf16(x1) if x1 is not None else None), _bf16(wt)
        y64 = kc._ref_fwd(self.case, x0, x1, wt, self.b, None)
        x = x0 if x1 is None else torch.cat([x0, x1], 1)
        if self.ups:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        t = F.conv2d(x.abs().double(), wt.abs().double(), self.b.abs().double(), padding=1)
        return y64, t


def _layer(be, tag):
    geom, ups = next((g, u) for t, g, u, _ in CASES if t == tag)
    return _Skinny(be, geom, ups, seed=len(tag))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("tag,geom,ups,pool", [c for c in CASES if not c[3]], ids=[c[0] for c in CASES if not c[3]])
def test_partials_sum_to_the_convolution_within_the_fp64_bound(rows64, tag, geom, ups, pool, prec):
    be = rows64
    bf = prec == "bf16"
    layer = _Skinny(be, geom, ups, seed=len(tag))
    n, h, w, c0, c1, cout = geom
    y64, t = layer.fp64(bf)
    seen = set()
    for s in SPLITS:
        with _Forced(be, (0, 0, s)):
            assert be.query("mnk_conv3x3_skinny_form", n, h, w, c0, c1, cout, ups | (BF16 if bf else 0), 0) == 1
            y = layer.y(BF16 if bf else 0)
            plan = kc._last_plan(be)
            seen.add(be.query("mnk_conv3x3_skinny_splits", n, h, w, c0, c1, cout))
        assert not torch.isnan(y).any(), (tag, s, "unwritten or NaN outputs")
        assert torch.all(y[..., cout:] == 0), (tag, s, "pad channels")
        ratio = float(((from_nhwc(y, cout).double() - y64).abs() / t.clamp_min(1e-30)).max())
        print("skinny fp64 %s %s %s splits %d: |y - y64| / T = %.3g (TAU %.3g)" % (be.kind, tag, prec, s, ratio, TAU))
        assert ratio <= TAU, (tag, prec, s, ratio)
        assert plan[0] == n * h * w and plan[1] == cout and plan[3] == 9 and plan[4] == 1 and plan[6] == 32, plan
    if c0 + c1 == 33:
        assert seen == {1, 2, 5}, ("K = 297 pads to 5 load rounds: 1, 2 and 5 splits are all taken", seen)
    assert 1 in seen and len(seen) >= 2, ("the forced split counts must reach the kernel", seen)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("tag,geom,ups,pool", CASES, ids=[c[0] for c in CASES])
def test_full_norm_epilogue_within_the_evalnorm_bound(rows64, tag, geom, ups, pool, prec):
    """|z - z64| <= |scale| TAU T + C 2^-24 (|scale| |y64 - mean| + |beta|), averaged over the pool window"""
    be = rows64
    bf = prec == "bf16"
    layer = _Skinny(be, geom, ups, seed=len(tag) + 3)
    n, h, w, c0, c1, cout = geom
    mean, scale, beta = _norm(cout, len(tag))
    assert bool((scale < 0).any()) and bool((scale > 0).any())
    y64, t = layer.fp64(bf)
    m, sc, b = (v.double()[None, :, None, None] for v in (mean, scale, beta))
    z64 = ((y64 - m) * sc + b).clamp_min(0)
    first, second = sc.abs() * TAU * t, 2.0 ** -24 * (sc.abs() * (y64 - m).abs() + b.abs())
    if pool:
        z64, first, second = (F.avg_pool2d(v, 2) for v in (z64, first, second))
    for s in SPLITS:
        with _Forced(be, (0, 0, s)):
            assert be.query("mnk_conv3x3_skinny_form", n, h, w, c0, c1, cout, ups | (BF16 if bf else 0), pool) == 1
            ws, splits = layer.partials(BF16 if bf else 0)
        z = layer.second_stage(ws, splits, mean, scale, beta, 1, pool)
        assert not torch.isnan(z).any()
        assert torch.all(z[..., cout:] == 0), (tag, s, "pad channels of z must be zero")
        err = (from_nhwc(z, cout).double() - z64).abs()
        print("skinny evalnorm %s %s %s splits %d: worst err / bound = %.3f"
              % (be.kind, tag, prec, splits, float((err / (first + C * second).clamp_min(1e-300)).max())))
        assert bool((err <= first + C * second).all()), (tag, prec, s)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_two_runs_are_bit_equal(rows64, prec):
    be = rows64
    flags = BF16 if prec == "bf16" else 0
    for tag in ("up-from-3x2", "all-padding-two-sources"):
        layer = _layer(be, tag)
        with _Forced(be, (0, 0, 5)):
            (a, sa), (b, sb) = layer.partials(flags), layer.partials(flags)
        assert sa == sb and torch.equal(a.cpu(), b.cpu()), tag


def test_bf16_pack_equals_the_fp32_pack_of_host_rounded_operands(rows64):
    """MNK_CONV_BF16 on the raw operands with the bf16 pack == the fp32 form on operands rounded to bf16 on the host (the same k
    reach the same thread in the same order, and a bf16 value is an fp32 value)"""
    be = rows64
    for tag in ("all-padding-two-sources", "up-from-2x2", "r12-partial-row-tile"):
        geom, ups = next((g, u) for t, g, u, _ in CASES if t == tag)
        raw = _Skinny(be, geom, ups, seed=7)
        pre = _Skinny(be, geom, ups, seed=7, prerounded=True)
        for s in SPLITS:
            with _Forced(be, (0, 0, s)):
                a, _ = raw.partials(BF16)
                b, _ = pre.partials(0)
            assert torch.equal(a.cpu(), b.cpu()), (tag, s, float((a.cpu() - b.cpu()).abs().max()))


def test_form_query_threshold_refusal_and_plan(be):
    from mnk._lib import MnkError
    be.lib.call("mnk_set_tuning", b"skinny_rows", 16)
    at = _Skinny(be, (1, 4, 4, 20, 0, 40), 0, seed=1)            # R = 16
    above = _Skinny(be, (17, 1, 1, 20, 0, 40), 0, seed=2)        # R = 17
    assert be.query("mnk_conv3x3_skinny_form", 1, 4, 4, 20, 0, 40, 0, 0) == 1
    assert be.query("mnk_conv3x3_skinny_form", 17, 1, 1, 20, 0, 40, 0, 0) == 0
    assert be.query("mnk_conv3x3_skinny_form", 1, 4, 4, 20, 0, 40, 16, 0) == 0      # MNK_CONV_BF16_TRAIN: no such form
    assert be.query("mnk_conv3x3_skinny_form", 1, 3, 3, 20, 0, 40, 0, 1) == 0       # an odd map cannot pool
    assert be.query("mnk_conv3x3_skinny_form", 1, 3, 3, 20, 0, 40, UPS, 0) == 0     # nor be an up-sampled one
    # the measured class rule (profiles/eval_skinny.txt): an up-sampled layer with fewer than skinny_up_min_weights (8 Mi) weights
    # keeps the sub-pixel launch, except a bf16 launch of at most 4 rows
    assert _DEFAULTS[be.kind][1] == 8 << 20
    assert be.query("mnk_conv3x3_skinny_form", 1, 2, 2, 1024, 10, 1024, UPS, 0) == 1
    assert be.query("mnk_conv3x3_skinny_form", 1, 2, 2, 1024, 0, 512, UPS, 0) == 0
    assert be.query("mnk_conv3x3_skinny_form", 1, 2, 2, 1024, 0, 512, UPS | BF16, 0) == 1
    assert be.query("mnk_conv3x3_skinny_form", 1, 4, 4, 1024, 0, 512, UPS | BF16, 0) == 0
    assert be.query("mnk_conv3x3_skinny_form", 1, 4, 4, 1024, 0, 512, 0, 1) == 1
    # the refused launch: MNK_EINVAL, nothing written
    n, h, w, c0, c1, cout = above.geom
    ws = be.empty(4 * n * h * w * ceil4(cout))
    with pytest.raises(MnkError, match="skinny_form answers 0"):
        be.call("mnk_conv3x3_skinny_fwd", *above._src(), 0, above.packs[0], n, h, w, cout, ws, ws.numel())
    be.sync()
    assert bool(torch.isnan(ws).all()), "a refused launch wrote to its workspace"
    # the taken launch reports itself
    with _Forced(be, (0, 0, 2)):
        _, splits = at.partials(0)
        plan = kc._last_plan(be)
    assert splits == 2 and plan == (16, 40, 3, 9, 1, 16, 32, 2), plan
    # nothing forced: the rule's split count is what the workspace query sizes and what runs
    _, splits = at.partials(0)
    assert kc._last_plan(be)[7] == splits >= 1
    # 0 switches the form off
    be.lib.call("mnk_set_tuning", b"skinny_rows", 0)
    assert be.query("mnk_conv3x3_skinny_form", 1, 1, 1, 20, 0, 40, 0, 0) == 0
