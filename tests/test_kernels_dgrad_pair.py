"""The pair form of the sub-pixel data gradient (mnk_conv3x3_up_dgrad_pair / _pair_bnstats; csrc/conv3x3.hip: ConvOut,
conv3x3_igemm_kernel<..., PAIR>, conv3x3_splitk_reduce_pair_kernel): the data gradients of an up-sampled convolution w.r.t. both of
its sources [x0 | x1] in one launch.  Every case runs the tuning value dgrad_pair = 0 (the two single launches) and 1 (the pair
entry) under the same plan and asks for equal bits -- both dx, the raw split-K partials, the statistics partials -- and checks dx
against the fp64 data gradient of conv2d(interpolate(x, 2, 'nearest')) at the tolerance of test_kernels_conv.py.
The same bodies run on the CPU emulator build (-m "not gpu") and on the MI355X (-m gpu)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import to_nhwc, from_nhwc, ceil4, relerr
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
import test_kernels_conv_tapskip as kts

TOL = 2e-6          # test_kernels_conv.py: every forward / data-gradient form against fp64
_FORCE = ("force_bm", "force_bn", "force_splits")


@pytest.fixture(autouse=True)
def tuning(be):
    """every launch that can skip taps walks position-major (the pay-off threshold ktap_skip_min is a measured value and may
    move); everything a case sets is put back"""
    v = ctypes.c_int()
    be.lib.call("mnk_get_tuning", b"ktap_skip_min", ctypes.addressof(v))
    be.lib.call("mnk_set_tuning", b"ktap_skip_min", 0)
    yield
    for name in _FORCE:
        be.lib.call("mnk_set_tuning", name.encode(), 0)
    be.lib.call("mnk_set_tuning", b"ktap_skip", 1)
    be.lib.call("mnk_set_tuning", b"ktap_skip_min", v.value)
    be.lib.call("mnk_set_tuning", b"dgrad_pair", 1)


def _last_plan(be):
    out = np.zeros(8, dtype=np.int64)
    be.lib.call("mnk_last_plan", out.ctypes.data)
    return tuple(int(v) for v in out)


_REF = {}


def _reference(n, h, w, cout, cs):
    """inputs and the fp64 data gradient of one shape, made once: (dy, weight, dx64 of the concatenated source, norm-layer records)"""
    key = (n, h, w, cout, cs)
    if key not in _REF:
        g = torch.Generator().manual_seed(41 + n + 7 * h + 11 * w + cout)
        cin = sum(cs)
        wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
        dy = torch.randn(n, cout, 2 * h, 2 * w, generator=g)
        x = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
        F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), wt.double(), None, padding=1).backward(dy.double())
        bns = []
        for c in cs:
            y = torch.randn(n, c, h, w, generator=g)
            mean, var = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
            invstd = (var + 1e-5).rsqrt()
            gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
            bns.append((to_nhwc(y), mean, invstd, gamma * invstd, beta))
        _REF[key] = (dy, wt, x.grad.detach(), bns)
    return _REF[key]


def _run_pair(be, n, h, w, cout, cs, bn):
    """the two single launches (dgrad_pair = 0), then the pair entry (1), under whatever plan is forced.
    -> {knob: ([dx0, dx1], [partials0, partials1] (None: no split), [stats0, stats1] (None: no record))}, the pair form, the split
    counts of the two sources"""
    dy, wt, dx64, bns = _reference(n, h, w, cout, cs)
    DY, Wt = be.t(to_nhwc(dy)), be.t(wt)
    ldy = DY.shape[-1]
    wd, starts = [], (0, cs[0])
    for c_start, c in zip(starts, cs):
        p = be.empty(be.query("mnk_conv3x3_up_dgrad_packed_floats", cout, c))
        be.call("mnk_conv3x3_up_pack_dgrad", Wt, p, cout, sum(cs), c_start, c)
        wd.append(p)
    recs = []
    for i, c in enumerate(cs):
        if bn[i]:
            y, mean, invstd, scale, beta = bns[i]
            recs.append((be.t(y), ceil4(c), be.t(mean), be.t(invstd), be.t(scale), be.t(beta), 0.0 if i == 0 else 0.2))
        else:
            recs.append(None)
    nws = [be.query("mnk_conv3x3_up_dgrad_workspace_floats", n, h, w, cout, c) for c in cs]
    nst = [be.query("mnk_conv3x3_up_dgrad_stats_floats", n, h, w, cout, c) if bn[i] else 0 for i, c in enumerate(cs)]
    assert all(v > 0 for v, b in zip(nst, bn) if b)
    out, splits = {}, []
    # ---- dgrad_pair = 0: the single entries -----------------------------------------------------------------------------------
    be.lib.call("mnk_set_tuning", b"dgrad_pair", 0)
    assert be.query("mnk_conv3x3_up_dgrad_pair_form", n, h, w, cout, cs[0], cs[1], int(bn[0]), int(bn[1])) == 0
    dxs, parts, sts = [], [], []
    for i, c in enumerate(cs):
        dx, ws = be.empty(n, h, w, ceil4(c)), be.empty(max(nws[i], 1))
        st = be.empty(nst[i]) if bn[i] else None
        if bn[i]:
            be.call("mnk_conv3x3_up_dgrad_bnstats", DY, ldy, cout, wd[i], dx, ceil4(c), n, h, w, c, ws, nws[i], st, *recs[i])
        else:
            be.call("mnk_conv3x3_up_dgrad", DY, ldy, cout, wd[i], dx, ceil4(c), n, h, w, c, ws, nws[i])
        be.sync()
        splits.append(_last_plan(be)[7])
        assert (nws[i] > 0) == (splits[i] > 1)
        dxs.append(dx.cpu()), parts.append(ws.cpu() if nws[i] else None), sts.append(st.cpu() if bn[i] else None)
    out[0] = (dxs, parts, sts)
    # ---- dgrad_pair = 1: the pair entry ---------------------------------------------------------------------------------------
    be.lib.call("mnk_set_tuning", b"dgrad_pair", 1)
    form = be.query("mnk_conv3x3_up_dgrad_pair_form", n, h, w, cout, cs[0], cs[1], int(bn[0]), int(bn[1]))
    assert be.query("mnk_conv3x3_up_dgrad_pair_workspace_floats", n, h, w, cout, cs[0], cs[1]) == sum(nws)
    full_nst = [be.query("mnk_conv3x3_up_dgrad_stats_floats", n, h, w, cout, c) for c in cs]
    assert be.query("mnk_conv3x3_up_dgrad_pair_stats_floats", n, h, w, cout, cs[0], cs[1]) == sum(full_nst)
    dxp = [be.empty(n, h, w, ceil4(c)) for c in cs]
    ws = be.empty(max(sum(nws), 1))
    stp = [be.empty(nst[i]) if bn[i] else None for i in range(2)]
    head = (DY, ldy, cout, wd[0], wd[1], dxp[0], ceil4(cs[0]), dxp[1], ceil4(cs[1]), n, h, w, cs[0], cs[1], ws, sum(nws))
    tail = ()
    for i in range(2):
        tail += (stp[i],) + (recs[i] if bn[i] else (None, 0, None, None, None, None, -1.0))

    def launch():
        if any(bn):
            be.call("mnk_conv3x3_up_dgrad_pair_bnstats", *head, *tail)
        else:
            be.call("mnk_conv3x3_up_dgrad_pair", *head)
        be.sync()
    if form == 0:
        # refused, nothing launched, nothing computed another way: the caller runs the two single launches
        from mnk._lib import MnkError
        with pytest.raises(MnkError):
            launch()
        assert all(bool(torch.isnan(d.cpu()).all()) for d in dxp), "a refused pair must not write"
        return out, form, splits
    launch()
    wsc = ws.cpu()
    out[1] = ([d.cpu() for d in dxp],
              [wsc[:nws[0]] if nws[0] else None, wsc[nws[0]:nws[0] + nws[1]] if nws[1] else None],
              [s.cpu() if s is not None else None for s in stp])
    return out, form, splits


def _check_equal(out, cs, n, h, w, cout):
    dx64 = _reference(n, h, w, cout, cs)[2]
    (dx0, ws0, st0), (dx1, ws1, st1) = out[0], out[1]
    c_start = 0
    for i, c in enumerate(cs):
        err = relerr(from_nhwc(dx1[i], c), dx64[:, c_start:c_start + c])
        print("source", i, "relerr vs fp64", err)
        assert torch.equal(dx1[i], dx0[i]), "dx of source %d" % i
        assert (ws1[i] is None) == (ws0[i] is None)
        if ws0[i] is not None:
            assert torch.equal(ws1[i], ws0[i]), "raw split-K partials of source %d" % i
        assert (st1[i] is None) == (st0[i] is None)
        if st0[i] is not None:
            assert torch.equal(st1[i], st0[i]), "statistics partials of source %d" % i
        assert err < TOL
        assert torch.all(dx1[i][..., c:] == 0), "pad channels of dx must be written as zero"
        c_start += c


def _force(be, plan):
    for name, v in zip(_FORCE, plan):
        be.lib.call("mnk_set_tuning", name.encode(), v)


N, COUT, CS = 3, 20, (70, 64)       # dy with 20 channels: a padded K chunk (32 K steps); 70 | 64: two tiles, the last one ragged
#                                     (ld 72), beside one full tile (ld 64)
MAPS = [(1, 1), (2, 2), (3, 5)]
PLANS = [(64, 64, 1), (64, 64, 3), (128, 64, 2)]      # 32 K steps in 3 splits: 11, 11, 10 -- the last split is shorter
RECORDS = [(False, False), (True, False), (True, True)]


@pytest.mark.parametrize("ktap_skip", [0, 1])
@pytest.mark.parametrize("bn", RECORDS, ids=["plain", "bn-first", "bn-both"])
@pytest.mark.parametrize("plan", PLANS, ids=lambda p: "%dx%d-s%d" % p)
@pytest.mark.parametrize("hw", MAPS, ids=lambda m: "%dx%d" % m)
def test_pair_equals_the_two_single_launches(be, hw, plan, bn, ktap_skip):
    h, w = hw
    be.lib.call("mnk_set_tuning", b"ktap_skip", ktap_skip)
    _force(be, plan)
    out, form, splits = _run_pair(be, N, h, w, COUT, CS, bn)
    assert splits == [plan[2], plan[2]]
    # Row order.  3 frames of a 2x2 or 3x5 map are one M tile that holds every position: no tap is outside for all of them and
    # both launches stay frame-major.  On the 1x1 map 12 of the 16 taps only read padding: a launch walks position-major unless
    # its epilogue leaves column sums (an unsplit launch with a record), so an unsplit pair with a record on ONE source has two
    # row orders and is not one launch.
    # The pair kernels exist for the 64-row tile in both row orders and for the 128-row tile frame-major.
    pm = [ktap_skip == 1 and hw == (1, 1) and not (plan[2] == 1 and b) for b in bn]
    refused = pm[0] != pm[1] or (pm[0] and plan[0] == 128)
    assert form == (0 if refused else 2 if plan[2] > 1 else 1), form
    if form:
        _check_equal(out, CS, N, h, w, COUT)


def test_pair_skips_taps_on_position_major_tiles(be):
    """40 frames of a 2x2 map on 64-row tiles: a tile holds two of the four positions and skips the taps that are outside for
    both -- three M tiles with different tap masks, in three splits, a record on both sources (the statistics come out of the
    one reduction)"""
    be.lib.call("mnk_set_tuning", b"ktap_skip", 1)
    _force(be, (64, 64, 3))
    n, h, w = 40, 2, 2
    be.lib.cdll.mnk_prof_reset()
    be.lib.cdll.mnk_prof_enable(1)
    try:
        out, form, splits = _run_pair(be, n, h, w, COUT, CS, (True, True))
    finally:
        be.lib.cdll.mnk_prof_enable(0)
    launches, ms, work, ex = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    be.lib.cdll.mnk_prof_query(0, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(work))          # group 0: conv3x3_igemm
    be.lib.cdll.mnk_prof_query_executed(0, ctypes.byref(ex))
    be.lib.cdll.mnk_prof_reset()
    assert form == 2 and splits == [3, 3]
    _check_equal(out, CS, n, h, w, COUT)
    # the recorder: two single launches + ONE pair launch, each half with the same algorithmic and executed work
    full = 2.0 * n * h * w * 16 * COUT * sum(CS)
    tiles = kts._tile_masks(64, n, h, w, 2 * h, 2 * w, 4, 4, 1, 2, 1)
    want = 2.0 * COUT * sum(CS) * sum(rows * bin(mask).count("1") for rows, mask in tiles)
    assert launches.value == 3
    assert work.value == 2 * (2.0 * 4.0 * n * h * w * 9.0 * COUT * sum(CS))
    assert want < full and ex.value == 2 * want, "the position-major tiles skip taps, the same in both halves"


def test_pair_with_the_rules_own_different_split_counts(be):
    """no forced plan: 8 frames of a 4x4 map (128 rows: two 64-row tiles) and 272 channels of dy (272 K steps) give the 70-wide
    source 4 tiles and the 64-wide one 2, and make_plan's rule for tiny problems splits them 55 and 68 times (mnk_last_plan): grid z
    is the larger count, and the blocks of the other source past its count leave at once.  One source splits into steps of 5, the
    other of 4; a record on the second source only."""
    n, h, w, cout = 8, 4, 4, 272
    out, form, splits = _run_pair(be, n, h, w, cout, CS, (False, True))
    print("split counts", splits)
    assert splits[0] != splits[1] and min(splits) > 1, splits
    assert form == 2
    _check_equal(out, CS, n, h, w, cout)


def test_pair_of_two_tile_families_is_refused(be):
    """70 | 16 channels: the second source's plan is the 16x16-MFMA kernel (BN = 16), the first one's a 32x32-MFMA tile -- no
    kernel serves both: the query answers 0, the pair entry is refused and writes nothing, and the two single launches are the
    data gradient"""
    cs = (70, 16)
    out, form, splits = _run_pair(be, N, 3, 5, COUT, cs, (False, False))
    assert form == 0 and 1 not in out
    dx64 = _reference(N, 3, 5, COUT, cs)[2]
    assert relerr(from_nhwc(out[0][0][0], 70), dx64[:, :70]) < TOL
    assert relerr(from_nhwc(out[0][0][1], 16), dx64[:, 70:]) < TOL


# ---- the autograd layer: Conv3x3Fn's backward issues the pair, with the _DZ_STATS hand-over of each source -------------------------
def _two_source_graph(be, n, knob):
    """[bn_act(conv(xa)) | bn_act(conv(xb))] at 8 x 8 -> up-sampled 3x3 convolution -> loss, from the public ops.
    -> (gradients of every leaf, DZ_STATS_COUNT, launches of the forward / data-gradient GEMM group)"""
    from mnk import ops
    from sync_batchnorm import SynchronizedBatchNorm3d
    ca, cb, c0, c1, co, hs = 5, 3, 52, 49, 20, 8
    g = torch.Generator().manual_seed(77)
    leaves = {"xa": be.t(torch.rand(n, ca, 1, hs, hs, generator=g)).requires_grad_(True),
              "xb": be.t(torch.rand(n, cb, 1, hs, hs, generator=g)).requires_grad_(True)}
    for k, shape in (("wa", (c0, ca, 1, 3, 3)), ("wb", (c1, cb, 1, 3, 3)), ("w", (co, c0 + c1, 1, 3, 3))):
        leaves[k] = torch.nn.Parameter(be.t(torch.randn(*shape, generator=g) * 0.2))
    leaves["b"] = torch.nn.Parameter(be.t(torch.randn(co, generator=g) * 0.1))
    norms = [SynchronizedBatchNorm3d(c, eps=1e-5).to(be.device).train() for c in (c0, c1)]
    gy = be.t(torch.randn(n, co, 1, 2 * hs, 2 * hs, generator=g))
    be.lib.call("mnk_set_tuning", b"dgrad_pair", knob)
    ops.clear_dz_stats()
    zs = []
    for x, w, c, cin, norm in ((leaves["xa"], leaves["wa"], c0, ca, norms[0]), (leaves["xb"], leaves["wb"], c1, cb, norms[1])):
        y, s = ops.conv3x3(ops.to_act(x), cin, w, None, want_stats=True)
        zs.append(ops.bn_act(y, c, norm, relu=True, sums=s))
    y, _ = ops.conv3x3(zs[0], c0, leaves["w"], leaves["b"], x1=zs[1], c1=c1, ups=True)
    loss = (ops.from_act(y, co, n) * gy).sum()
    ops.DZ_STATS_COUNT[0] = ops.DZ_STATS_COUNT[1] = 0
    be.lib.cdll.mnk_prof_reset()
    be.lib.cdll.mnk_prof_enable(1)
    try:
        loss.backward()
        be.sync()
    finally:
        be.lib.cdll.mnk_prof_enable(0)
    launches, ms, work = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double()
    be.lib.cdll.mnk_prof_query(0, ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(work))          # group 0: conv3x3_igemm
    be.lib.cdll.mnk_prof_reset()
    assert ops.handover_state() == {}, ops.handover_state()
    grads = {k: v.grad.detach().cpu().clone() for k, v in leaves.items()}
    for i, norm in enumerate(norms):
        grads["gamma%d" % i], grads["beta%d" % i] = norm.weight.grad.detach().cpu().clone(), norm.bias.grad.detach().cpu().clone()
    return grads, tuple(ops.DZ_STATS_COUNT), launches.value


def test_backward_of_a_two_source_up_sampled_convolution_issues_the_pair(be):
    """both sources are outputs of training-mode norm layers with more rows than the one-launch norm kernels take: the data gradient
    of the up-sampled convolution is one launch that also leaves both layers' backward statistics, both hand-overs are taken, and
    every gradient of the graph keeps its bits"""
    n = be.query("mnk_bn_small_rows") // 64 + 1
    assert be.query("mnk_conv3x3_up_dgrad_pair_form", n, 8, 8, 20, 52, 49, 1, 1) > 0
    g0, count0, launches0 = _two_source_graph(be, n, 0)
    g1, count1, launches1 = _two_source_graph(be, n, 1)
    print("DZ_STATS_COUNT", count0, count1, "GEMM launches of the backward pass", launches0, "->", launches1)
    assert count0 == count1 == (2, 0), "both norm layers take the hand-over of their backward statistics"
    assert launches1 == launches0 - 1
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
