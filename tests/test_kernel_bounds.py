"""Memory behaviour and launch plans of the GEMM kernels, on guard-banded buffers (tests/_guard.py):

* workspace honesty: every entry point that takes (ws, ws_floats), at a shape whose plan uses the workspace, runs with exactly
  the queried size and with one float less (inside a guard band of the full size): the first must be correct with intact
  guards, the second must raise MnkError or be correct with intact guards;
* forced launch plans (force_bm / force_bn / force_splits) on every GEMM form -- 3x3 forward with two sources and a residual,
  sub-pixel forward (with and without statistics) and data gradient, the two _bnstats data gradients, the K x K forms -- at
  shapes whose M and Cout are ragged with respect to every block tile: the reported plan, the values against fp64 per element,
  the fused statistics, dx of the _bnstats launches against the plain launch, pad channels;
* (MI355X) every row of csrc/plan_table.h and plan_table_bf16x3.h at its own shape: the table's plan is the one that runs, and
  it computes the convolution.

Per-element criterion: |y - y64| <= TAU * (|x| (*) |w| + |bias| + |residual|), (*) the same convolution on absolute values --
the size of every term the fp32 chain adds, so the bound holds for any K and any split of it."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from _util import to_nhwc, from_nhwc, ceil4
import test_kernels_bn as kbn
import test_kernels_conv as kc
import test_kernels_conv1x1_fast as k11
import test_kernels_motion as kmo
import test_multiframe_kernels as kmf
import test_predictor as kpr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monkey-net_amd", "csrc")

# worst |y - y64| / (|x| (*) |w| + |b| + |r|) measured in both GEMM modes: 2.8e-7 (MI355X) / 4.4e-7 (emulator) over the forced
# plans below, 4.0e-7 over the plan-table rows on the MI355X (K up to 2064 x 4) -- a few units of fp32 rounding (2^-24 = 6e-8)
# on the magnitude of the terms added.  TAU = 1.8x the worst, the same in both modes.
TAU = 8e-7

_MODES = ("gemm_bf16x3", "wgrad_bf16x3", "gemm16_bf16x3")
_FORCE = ("force_bm", "force_bn", "force_splits")


@pytest.fixture(params=["f32-mfma", "bf16x3"])
def mode(request, be):
    on = 1 if request.param == "bf16x3" else 0
    try:
        for k in _MODES:
            be.lib.call("mnk_set_tuning", k.encode(), on)
        yield on
    finally:
        for k in _MODES:
            be.lib.call("mnk_set_tuning", k.encode(), 0)


# ---- 3. workspace honesty ---------------------------------------------------------------------------------------------------
# (id, body on a backend, entry points that must have run with a non-empty workspace).  Bodies are the kernel tests of the
# family at a shape whose plan splits (or otherwise uses the workspace); their own assertions judge the output.
WS_CASES = [
    ("conv3x3-fwd-splitk", lambda be: kc.test_conv3x3_forward(be, (3, 4, 4, 40, 0, 136, 0, False, False), True), {"mnk_conv3x3_fwd"}),
    ("subpixel-fwd-dgrad", lambda be: kc.test_conv3x3_upsampled_subpixel_forward_and_dgrad(be, kc.UP_CASES[0]),
     {"mnk_conv3x3_up_fwd", "mnk_conv3x3_up_dgrad"}),
    ("kxk-4x4-fwd-dgrad", lambda be: kc.test_conv4x4_nopad_forward_dgrad_wgrad(be, (3, 6, 6, 64, 20), 2), {"mnk_conv2d_fwd"}),
    ("dgrad-bnstats-splitk", lambda be: kc.test_data_gradient_leaves_the_backward_statistics_of_the_norm_layer_in_front(
        be, kc.BNSTATS_CASES[4]), {"mnk_conv3x3_dgrad_bnstats"}),
    ("wgrad-halo", lambda be: kc.test_conv3x3_wgrad(be, kc.HALO_CASES[2], False), {"mnk_conv3x3_wgrad"}),
    ("wgrad-gather", lambda be: kc.test_conv3x3_wgrad(be, kc.HALO_CASES[9], False), {"mnk_conv3x3_wgrad"}),
    ("wgrad-n16", lambda be: kc.test_conv3x3_wgrad(be, kc.HALO_CASES[10], True), {"mnk_conv3x3_wgrad"}),
    ("wgrad-tapmajor", lambda be: kc.test_conv3x3_wgrad(be, kc.HALO_CASES[8], True), {"mnk_conv3x3_wgrad"}),
    ("wgrad-compact", lambda be: kc.test_conv3x3_wgrad(be, kc.COMPACT_CASES[4], True), {"mnk_conv3x3_wgrad"}),
    ("wgrad-subpixel", lambda be: kc.test_conv3x3_wgrad(be, kc.COMPACT_CASES[8], True), {"mnk_conv3x3_wgrad"}),
    ("bn-stats-and-backward", lambda be: kbn.test_bn_train_forward_backward(be, (1, 64, 16, 16), 1),
     {"mnk_bn_stats", "mnk_bn_act_bwd_stats"}),
    ("bn-small-split-partials", lambda be: kbn.test_bn_small_sums_the_split_k_partials_of_the_convolution_in_front(be, 1),
     {"mnk_conv3x3_up_fwd"}),
    ("norm-stats", lambda be: kbn.test_instance_norm_leaky_pool(be, (2, 70, 6, 5), 1), {"mnk_norm_stats"}),
    ("gconv1x1-weight", lambda be: kmo.test_gconv1x1(be, 11, 4), {"mnk_gconv1x1_bwd_weight"}),
    ("conv1x1-weight", lambda be: kmo.test_conv1x1_sigmoid(be, 70, 4, 1, (6, 5)), {"mnk_conv1x1_sigmoid_bwd"}),
    ("deform-backward", lambda be: kmo.test_deform(be, "wide", (2, 300, 4, 4), 0), {"mnk_deform_bwd"}),
    ("gru-gemm-splitk", lambda be: kpr.test_gemm_against_fp64(be, 1, 0, 40, 24, 1100, False), {"mnk_gru_gemm"}),
    ("gru-colsum", lambda be: kpr.test_colsum_against_fp64(be), {"mnk_gru_colsum"}),
    # the warps of all levels in one launch; C = 300 takes channel slices, i.e. the most workspace per pixel
    ("warp-levels-backward", lambda be: kmo.test_warp_levels_direct(be, "edges", 0, "all"), {"mnk_warp_levels_bwd"}),
    ("warp-levels-shared-backward", lambda be: kmf.test_shared_source_equals_the_repeated_source_all_levels(be, *kmf.SHARED_CASES[4]),
     {"mnk_warp_levels_shared_bwd"}),
    ("deform-shared-backward", lambda be: kmf.test_shared_source_equals_the_repeated_source_per_level(be, *kmf.SHARED_CASES[4]),
     {"mnk_deform_shared_bwd"}),
    ("bn-apply-colsum", lambda be: kbn.test_bn_train_forward_backward(be, (3, 45, 4, 6), 0), {"mnk_bn_act_bwd_apply_colsum"}),
    ("bn-apply-add-colsum", lambda be: kbn.test_bn_backward_apply_adds_the_skip_gradient(be, (1, 64, 16, 16), 1),
     {"mnk_bn_act_bwd_apply_add_colsum"}),
    ("bn-stats-finalize", lambda be: kbn.test_bn_train_forward_backward(be, (2, 300, 2, 2), 0), {"mnk_bn_stats_finalize"}),
    ("norm-backward-stats", lambda be: kbn.test_instance_norm_leaky_pool(be, (3, 12, 13, 13), 0), {"mnk_norm_act_bwd_stats"}),
    ("conv1x1-head-two-row-blocks", lambda be: k11.test_head_weight_gradient_with_one_and_with_two_row_blocks(
        be, (18, 11), 70, 0, 2, 0), {"mnk_conv1x1_bwd"}),
    ("kxk-4x4-wgrad", lambda be: kc.test_conv4x4_nopad_forward_dgrad_wgrad(be, kc.K4_CASES[0], 0), {"mnk_conv2d_wgrad"}),
    # the sub-pixel data gradient at BNSTATS_CASES[4]'s sizes: few tiles and K = 16 taps x 9 chunks, so the plan splits K
    ("subpixel-dgrad-bnstats-splitk", lambda be: kc.test_data_gradient_leaves_the_backward_statistics_of_the_norm_layer_in_front(
        be, (2, 4, 4, 136, 24, True, False, 0.0)), {"mnk_conv3x3_up_dgrad_bnstats"}),
]


@pytest.mark.parametrize("shrink", [0, 1], ids=["queried-size", "one-float-less"])
@pytest.mark.parametrize("tag,body,entries", WS_CASES, ids=[c[0] for c in WS_CASES])
def test_workspace_queries_cover_what_the_kernels_write(be, mode, tag, body, entries, shrink):
    be.ws_shrink = shrink
    body(be)
    seen = {name for name, _, _ in be.ws_log}
    assert entries <= seen, ("these entry points never ran with a workspace here", entries - seen, be.ws_log)
    print(tag, sorted(set(be.ws_log)))


# ---- 4. forced plans on every GEMM form -------------------------------------------------------------------------------------
TILES = [(64, 64), (64, 128), (128, 64), (128, 128), (128, 32), (128, 16), (128, 48)]


def _tile_ok(bm, bn, cout, phases):
    """conv3x3.hip plan_tile_ok under default tuning (mfma16 = 1, gemm_bf16x3_n48 = 0)"""
    if bn in (16, 48):
        return bm == 128 and phases == 1 and cout <= bn
    if bn == 32:
        return bm == 128
    return bn in (64, 128) and bm in (64, 128)


def _norm_splits(s, ksteps):
    per = -(-ksteps // min(s, ksteps))
    return -(-ksteps // per)


def _plans(ksteps, tile):
    """every tile with 1 and 3 splits, every split count (1, 2, 3, 5, ksteps, ksteps + 3) on `tile`"""
    out = [(bm, bn, s) for bm, bn in TILES for s in (1, 3)]
    out += [tile + (s,) for s in (2, 5, ksteps, ksteps + 3)]
    return out


class _Forced:
    def __init__(self, be, plan):
        self.be, self.plan = be, plan

    def __enter__(self):
        for k, v in zip(_FORCE, self.plan):
            self.be.lib.call("mnk_set_tuning", k.encode(), v)

    def __exit__(self, *exc):
        for k in _FORCE:
            self.be.lib.call("mnk_set_tuning", k.encode(), 0)


def _check_plan(be, plan, cout, taps, phases, ksteps):
    got = kc._last_plan(be)
    bm, bn, s = plan
    assert got[1] == cout and got[3] == taps and got[4] == phases and got[2] * got[3] == ksteps, (got, plan)
    if _tile_ok(bm, bn, cout, phases):
        assert got[5:7] == (bm, bn), ("forced tile not taken", got, plan)
    else:
        assert got[5:7] != (bm, bn), ("a tile without an instantiation was taken", got, plan)
    assert got[7] == _norm_splits(s, ksteps), ("split count", got, plan)
    return got


def _ratio(y, y64, bound):
    err = (y.double() - y64).abs()
    return float((err / bound.clamp_min(1e-30)).max())


def _check_values(y, y64, bound, what):
    r = _ratio(y, y64, bound)
    assert r <= TAU, ("%s: |y - y64| / (|x| (*) |w|) = %.3g > %.3g" % (what, r, TAU))
    return r


def _check_sums(sums, y64, c, what):
    """finished [sum y | sum y^2] per channel against fp64, relative to the sums of magnitudes"""
    want = torch.cat([y64.sum(dim=(0, 2, 3)), (y64 * y64).sum(dim=(0, 2, 3))])
    mag = torch.cat([y64.abs().sum(dim=(0, 2, 3)), (y64 * y64).sum(dim=(0, 2, 3))])
    err = (sums.cpu().double()[:2 * c] - want).abs()
    assert bool((err <= 1e-5 * mag + 1e-6).all()), (what, float((err / (mag + 1e-30)).max()))


def _dgrad_bnstats_ref(dz, y, mean, invstd, scale, beta, slope):
    d = y.double() - mean.double()[None, :, None, None]
    pre = d * scale.double()[None, :, None, None] + beta.double()[None, :, None, None]
    gg = dz if slope < 0 else torch.where(pre > 0, dz, dz * slope)
    want = torch.cat([gg.sum(dim=(0, 2, 3)), (gg * d * invstd.double()[None, :, None, None]).sum(dim=(0, 2, 3))])
    mag = torch.cat([gg.abs().sum(dim=(0, 2, 3)), (gg * d * invstd.double()[None, :, None, None]).abs().sum(dim=(0, 2, 3))])
    return want, mag


def _bn_inputs(g, n, c, h, w):
    y = torch.randn(n, c, h, w, generator=g)
    mean, var = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
    invstd = (var + 1e-5).rsqrt()
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    return y, mean, invstd, gamma * invstd, beta


def _stats_dgrad(be, st, nst, ldx, c, dz, bn, slope):
    sums = be.empty(2 * c)
    be.call("mnk_bn_stats_finish", st, nst // (2 * ldx), ldx, c, sums)
    be.sync()
    y, mean, invstd, scale, beta = bn
    want, mag = _dgrad_bnstats_ref(dz, y, mean, invstd, scale, beta, slope)
    err = (sums.cpu().double() - want).abs()
    assert bool((err <= 2e-5 * mag + 1e-6).all()), float((err / (mag + 1e-30)).max())


@pytest.mark.parametrize("cout", [40, 136])
def test_forced_plans_3x3_forward_two_sources_residual(be, mode, cout):
    n, h, w, c0, c1 = 2, 5, 7, 20, 13                         # M = 70, 3 chunks
    case = (n, h, w, c0, c1, cout, 0, True, True)
    x0, x1, wt, b, r = kc._inputs(case, seed=21)
    y64 = kc._ref_fwd(case, x0, x1, wt, b, r)
    bound = F.conv2d(torch.cat([x0, x1], 1).abs().double(), wt.abs().double(), b.abs().double(), padding=1) + r.abs().double()
    wp = be.empty(be.query("mnk_conv3x3_packed_floats", cout, c0, c1))
    be.call("mnk_conv3x3_pack_fwd", be.t(wt), wp, cout, c0, c1)
    X0, X1, R, B = be.t(to_nhwc(x0)), be.t(to_nhwc(x1)), be.t(to_nhwc(r)), be.t(b)
    ldy, ksteps = ceil4(cout), 9 * 3
    worst = 0.0
    for plan in _plans(ksteps, (128, 32)):
        with _Forced(be, plan):
            nws = be.query("mnk_conv3x3_workspace_floats", n, h, w, c0, c1, cout)
            nst = be.query("mnk_conv3x3_stats_floats", n, h, w, c0, c1, cout)
            Y = be.empty(n, h, w, ldy)
            ws = be.empty(nws) if nws else None
            st = be.empty(nst) if nst else None
            be.call("mnk_conv3x3_fwd", X0, X0.shape[-1], c0, X1, X1.shape[-1], c1, 2, wp, B, R, R.shape[-1], Y, ldy, n, h, w, cout,
                    ws, nws, st)
            be.sync()
            _check_plan(be, plan, cout, 9, 1, ksteps)
        Yc = Y.cpu()
        worst = max(worst, _check_values(from_nhwc(Yc, cout), y64, bound, plan))
        assert torch.all(Yc[..., cout:] == 0), plan
        if nst:
            sums = be.empty(2 * cout)
            be.call("mnk_bn_stats_finish", st, nst // (2 * ldy), ldy, cout, sums)
            be.sync()
            _check_sums(sums, y64, cout, plan)
    print("worst ratio", worst)


@pytest.mark.parametrize("with_stats", [False, True])
def test_forced_plans_subpixel_forward(be, mode, with_stats):
    n, h, w, c0, cout = 2, 5, 7, 40, 70                       # M = 70 per phase, 3 chunks
    g = torch.Generator().manual_seed(22)
    x = torch.randn(n, c0, h, w, generator=g)
    wt = torch.randn(cout, c0, 3, 3, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    xu = F.interpolate(x.double(), scale_factor=2, mode="nearest")
    y64 = F.conv2d(xu, wt.double(), b.double(), padding=1)
    bound = F.conv2d(xu.abs(), wt.abs().double(), b.abs().double(), padding=1)
    wp = be.empty(be.query("mnk_conv3x3_up_packed_floats", cout, c0, 0))
    be.call("mnk_conv3x3_up_pack_fwd", be.t(wt), wp, cout, c0, 0)
    X, B = be.t(to_nhwc(x)), be.t(b)
    ldy, ksteps = ceil4(cout), 4 * 3
    worst = 0.0
    for plan in _plans(ksteps, (64, 128)):
        with _Forced(be, plan):
            nws = be.query("mnk_conv3x3_up_workspace_floats", n, h, w, c0, 0, cout)
            nst = be.query("mnk_conv3x3_up_stats_floats", n, h, w, c0, 0, cout) if with_stats else 0
            Y = be.empty(n, 2 * h, 2 * w, ldy)
            ws = be.empty(nws) if nws else None
            st = be.empty(nst) if nst else None
            be.call("mnk_conv3x3_up_fwd", X, X.shape[-1], c0, None, 0, 0, 0, wp, B, Y, ldy, n, h, w, cout, ws, nws, st)
            be.sync()
            _check_plan(be, plan, cout, 4, 4, ksteps)
        Yc = Y.cpu()
        worst = max(worst, _check_values(from_nhwc(Yc, cout), y64, bound, plan))
        assert torch.all(Yc[..., cout:] == 0), plan
        if nst:
            sums = be.empty(2 * cout)
            be.call("mnk_bn_stats_finish", st, nst // (2 * ldy), ldy, cout, sums)
            be.sync()
            _check_sums(sums, y64, cout, plan)
    print("worst ratio", worst)


def _dgrad_refs(dy, wt, up):
    """fp64 dx of conv2d(x, w, pad 1) (through the nearest x2 up-sampling when up) and the same on absolute values"""
    n, _, ho, wo = dy.shape
    c = wt.shape[1]
    out = []
    for d, k in ((dy.double(), wt.double()), (dy.abs().double(), wt.abs().double())):
        gx = torch.nn.grad.conv2d_input((n, c, ho, wo), k, d, padding=1)
        out.append(F.avg_pool2d(gx, 2) * 4 if up else gx)
    return out


@pytest.mark.parametrize("form", ["3x3-dgrad-bnstats", "subpixel-dgrad", "subpixel-dgrad-bnstats"])
def test_forced_plans_data_gradients(be, mode, form):
    """the data-gradient GEMMs under every forced plan: dx against fp64 per element; the _bnstats launches leave the same dx to
    the bit as the plain launch under the same plan, and statistics that match fp64"""
    up = form.startswith("subpixel")
    stats = form.endswith("bnstats")
    n, h, w = 2, 5, 7                                          # dx geometry; M = 70
    cout, c, slope = (33, 136, 0.0) if form == "subpixel-dgrad-bnstats" else ((40, 13, -1.0) if up else (40, 70, 0.2))
    g = torch.Generator().manual_seed(23 + len(form))
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    dy = torch.randn(n, cout, ho, wo, generator=g)
    wt = torch.randn(cout, c, 3, 3, generator=g) * 0.2
    res = torch.randn(n, c, h, w, generator=g) if not up else None
    dx64, bound = _dgrad_refs(dy, wt, up)
    if res is not None:
        dx64, bound = dx64 + res.double(), bound + res.abs().double()
    bn = _bn_inputs(g, n, c, h, w)
    DY, ldx = be.t(to_nhwc(dy)), ceil4(c)
    BN = (be.t(to_nhwc(bn[0])), ldx) + tuple(be.t(v) for v in bn[1:]) + (float(slope),)
    R = be.t(to_nhwc(res)) if res is not None else None
    if up:
        wp = be.empty(be.query("mnk_conv3x3_up_dgrad_packed_floats", cout, c))
        be.call("mnk_conv3x3_up_pack_dgrad", be.t(wt), wp, cout, c, 0, c)
        taps, ksteps = 16, 16 * ((cout + 15) // 16)
    else:
        wp = be.empty(be.query("mnk_conv3x3_packed_floats", c, cout, 0))
        be.call("mnk_conv3x3_pack_dgrad", be.t(wt), wp, cout, c, 0, c)
        taps, ksteps = 9, 9 * ((cout + 15) // 16)
    worst = 0.0
    for plan in _plans(ksteps, (128, 64)):
        with _Forced(be, plan):
            if up:
                nws = be.query("mnk_conv3x3_up_dgrad_workspace_floats", n, h, w, cout, c)
                nst = be.query("mnk_conv3x3_up_dgrad_stats_floats", n, h, w, cout, c) if stats else 0
            else:
                nws = be.query("mnk_conv3x3_workspace_floats", n, h, w, cout, 0, c)
                nst = be.query("mnk_conv3x3_stats_floats", n, h, w, cout, 0, c)
            ws = be.empty(nws) if nws else None
            dx_a = be.empty(n, h, w, ldx)
            if up:
                be.call("mnk_conv3x3_up_dgrad", DY, DY.shape[-1], cout, wp, dx_a, ldx, n, h, w, c, ws, nws)
            else:
                be.call("mnk_conv3x3_fwd", DY, DY.shape[-1], cout, None, 0, 0, 2, wp, None, R, ldx, dx_a, ldx, n, h, w, c, ws, nws,
                        None)
            be.sync()
            _check_plan(be, plan, c, taps, 1, ksteps)
            if stats and nst:
                dx_b, st = be.empty(n, h, w, ldx), be.empty(nst)
                if up:
                    be.call("mnk_conv3x3_up_dgrad_bnstats", DY, DY.shape[-1], cout, wp, dx_b, ldx, n, h, w, c, ws, nws, st, *BN)
                else:
                    be.call("mnk_conv3x3_dgrad_bnstats", DY, DY.shape[-1], cout, wp, R, ldx, dx_b, ldx, n, h, w, c, ws, nws, st, *BN)
                be.sync()
                _check_plan(be, plan, c, taps, 1, ksteps)
                assert torch.equal(dx_a.cpu(), dx_b.cpu()), ("the _bnstats launch changed dx", plan)
                _stats_dgrad(be, st, nst, ldx, c, from_nhwc(dx_a.cpu(), c).double(), bn, slope)
        D = dx_a.cpu()
        worst = max(worst, _check_values(from_nhwc(D, c), dx64, bound, plan))
        assert torch.all(D[..., c:] == 0), plan
    print("worst ratio", worst)


# (n, hi, wi, cin, cout, k, pad, direction): 4x4 pad 0 forward, its pad-3 data gradient, 5x5 pad 2
KXK_FORCED = [(2, 10, 11, 36, 40, 4, 0, "fwd"), (2, 10, 11, 36, 40, 4, 3, "dgrad"), (2, 9, 8, 35, 70, 5, 2, "fwd")]


@pytest.mark.parametrize("loader", [0, 2], ids=["generic-loader", "kxk-buffer-loader"])
@pytest.mark.parametrize("case", KXK_FORCED, ids=["4x4-pad0", "4x4-pad3-dgrad", "5x5-pad2"])
def test_forced_plans_kxk(be, mode, case, loader):
    n, hi, wi, cin, cout, k, pad, direction = case
    g = torch.Generator().manual_seed(24 + k + pad)
    wt = torch.randn(cout, cin, k, k, generator=g) * 0.2
    if direction == "fwd":
        x = torch.randn(n, cin, hi, wi, generator=g)
        b = torch.randn(cout, generator=g)
        y64 = F.conv2d(x.double(), wt.double(), b.double(), padding=pad)
        bound = F.conv2d(x.abs().double(), wt.abs().double(), b.abs().double(), padding=pad)
        c_in, c_out, kw_ = cin, cout, wt
        wp = be.empty(be.query("mnk_conv2d_packed_floats", cout, cin, 0, k * k))
        be.call("mnk_conv2d_pack_fwd", be.t(wt), wp, cout, cin, 0, k * k)
        B = be.t(b)
    else:                     # dx of the pad-0 forward = the same kernel on dy with pad k - 1 and the flipped pack
        ho, wo = hi - k + 1, wi - k + 1
        x = torch.randn(n, cout, ho, wo, generator=g)       # dy
        y64 = torch.nn.grad.conv2d_input((n, cin, hi, wi), wt.double(), x.double())
        bound = torch.nn.grad.conv2d_input((n, cin, hi, wi), wt.abs().double(), x.abs().double())
        c_in, c_out = cout, cin
        wp = be.empty(be.query("mnk_conv2d_packed_floats", cin, cout, 0, k * k))
        be.call("mnk_conv2d_pack_dgrad", be.t(wt), wp, cout, cin, 0, cin, k * k)
        B = None
    ho, wo = y64.shape[2], y64.shape[3]
    hin, win = x.shape[2], x.shape[3]
    X, ldy, ksteps = be.t(to_nhwc(x)), ceil4(c_out), k * k * ((c_in + 15) // 16)
    worst = 0.0
    for plan in _plans(ksteps, (64, 64)):
        with _Forced(be, plan):
            nws = be.query("mnk_conv2d_workspace_floats", n, ho, wo, c_in, 0, c_out, k * k)
            ws = be.empty(nws) if nws else None
            Y = be.empty(n, ho, wo, ldy)
            be.call("mnk_conv2d_fwd", X, X.shape[-1], c_in, None, 0, 0, loader, hin, win, k, k, pad, wp, B, None, 0, Y, ldy, n, ho,
                    wo, c_out, ws, nws, None)
            be.sync()
            _check_plan(be, plan, c_out, k * k, 1, ksteps)
        Yc = Y.cpu()
        worst = max(worst, _check_values(from_nhwc(Yc, c_out), y64, bound, plan))
        assert torch.all(Yc[..., c_out:] == 0), plan
    print("worst ratio", worst)


# ---- 5. every plan-table row at its own shape (MI355X) ----------------------------------------------------------------------
def _table_rows(fname):
    rows = []
    for line in open(os.path.join(CSRC, fname)):
        m = re.match(r"\s*\{([-\d,\s]+)\},\s*//\s*(.*)", line)
        if m:
            v = [int(t) for t in m.group(1).split(",")]
            rows.append(("%s:%s" % (fname, m.group(2).split(":")[0].strip().replace(" ", "-")), tuple(v)))
    return rows


TABLE_ROWS = [(f, i, name, v) for f in ("plan_table.h", "plan_table_bf16x3.h") for i, (name, v) in enumerate(_table_rows(f))]


def _lookup(key, bf16x3):
    """the row make_plan takes for key = (M, Cout, chunks, taps, phases) under gemm_bf16x3 = bf16x3"""
    order = ("plan_table_bf16x3.h", "plan_table.h") if bf16x3 else ("plan_table.h",)
    for f in order:
        for ff, _, _, v in TABLE_ROWS:
            if ff == f and v[:5] == key:
                return v
    return None


def _factor(m):
    h = int(math.isqrt(m))
    while m % h:
        h -= 1
    return 1, h, m // h


_REF_CACHE = {}


def _row_problem(v, seed):
    """inputs and the fp64 reference of a table row's problem (cached: both modes use it)"""
    if v in _REF_CACHE:
        return _REF_CACHE[v]
    M, cout, chunks, taps, phases = v[:5]
    n, h, w = _factor(M)
    cin = 16 * chunks - 3                                   # ragged inside the last chunk, same chunk count
    g = torch.Generator().manual_seed(seed)
    threads = torch.get_num_threads()
    torch.set_num_threads(16)
    try:
        if taps == 16:                                      # sub-pixel data gradient: dy has cin channels at (2h, 2w)
            dy = torch.randn(n, cin, 2 * h, 2 * w, generator=g)
            wt = torch.randn(cin, cout, 3, 3, generator=g) * 0.2
            y64, bound = _dgrad_refs(dy, wt, True)
            prob = (dy, wt, None)
        else:
            x = torch.randn(n, cin, h, w, generator=g)
            wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
            b = torch.randn(cout, generator=g)
            xs = F.interpolate(x.double(), scale_factor=2, mode="nearest") if phases == 4 else x.double()
            y64 = F.conv2d(xs, wt.double(), b.double(), padding=1)
            bound = F.conv2d(xs.abs(), wt.abs().double(), b.abs().double(), padding=1)
            prob = (x, wt, b)
    finally:
        torch.set_num_threads(threads)
    _REF_CACHE.clear()                                      # one row at a time: the two modes of a row run back to back
    _REF_CACHE[v] = ((n, h, w, cin), prob, y64, bound)
    return _REF_CACHE[v]


@pytest.mark.gpu
@pytest.mark.parametrize("bf16x3", [0, 1], ids=["f32-mfma", "bf16x3"])
@pytest.mark.parametrize("fname,idx,name,row", TABLE_ROWS, ids=["%s#%d:%s" % (f, i, n.split(":")[1]) for f, i, n, _ in TABLE_ROWS])
def test_every_plan_table_row_runs_its_plan_and_computes_the_convolution(make_backend, fname, idx, name, row, bf16x3):
    from _guard import guarded
    be = guarded(make_backend("hip"))
    M, cout, chunks, taps, phases = row[:5]
    want = _lookup(row[:5], bf16x3)
    (n, h, w, cin), (x, wt, b), y64, bound = _row_problem(row, 1000 + idx)
    try:
        for k in _MODES:
            be.lib.call("mnk_set_tuning", k.encode(), bf16x3)
        W = be.t(wt)
        if taps == 16:
            wp = be.empty(be.query("mnk_conv3x3_up_dgrad_packed_floats", cin, cout))
            be.call("mnk_conv3x3_up_pack_dgrad", W, wp, cin, cout, 0, cout)
            nws = be.query("mnk_conv3x3_up_dgrad_workspace_floats", n, h, w, cin, cout)
            DY, ld = be.t(to_nhwc(x)), ceil4(cout)
            Y = be.empty(n, h, w, ld)
            ws = be.empty(nws) if nws else None
            be.call("mnk_conv3x3_up_dgrad", DY, DY.shape[-1], cin, wp, Y, ld, n, h, w, cout, ws, nws)
        elif phases == 4:
            wp = be.empty(be.query("mnk_conv3x3_up_packed_floats", cout, cin, 0))
            be.call("mnk_conv3x3_up_pack_fwd", W, wp, cout, cin, 0)
            nws = be.query("mnk_conv3x3_up_workspace_floats", n, h, w, cin, 0, cout)
            X, ld = be.t(to_nhwc(x)), ceil4(cout)
            Y = be.empty(n, 2 * h, 2 * w, ld)
            ws = be.empty(nws) if nws else None
            be.call("mnk_conv3x3_up_fwd", X, X.shape[-1], cin, None, 0, 0, 0, wp, be.t(b), Y, ld, n, h, w, cout, ws, nws, None)
        else:
            wp = be.empty(be.query("mnk_conv3x3_packed_floats", cout, cin, 0))
            be.call("mnk_conv3x3_pack_fwd", W, wp, cout, cin, 0)
            nws = be.query("mnk_conv3x3_workspace_floats", n, h, w, cin, 0, cout)
            X, ld = be.t(to_nhwc(x)), ceil4(cout)
            Y = be.empty(n, h, w, ld)
            ws = be.empty(nws) if nws else None
            be.call("mnk_conv3x3_fwd", X, X.shape[-1], cin, None, 0, 0, 2, wp, be.t(b), None, 0, Y, ld, n, h, w, cout, ws, nws, None)
        be.sync()
        got = kc._last_plan(be)
    finally:
        for k in _MODES:
            be.lib.call("mnk_set_tuning", k.encode(), 0)
    assert got[:5] == row[:5], (name, got)
    if want is not None:
        ksteps = chunks * taps
        assert got[5:] == (want[5], want[6], _norm_splits(want[7], ksteps)), ("the table's plan did not run", name, got, want)
    Yc = Y.cpu()
    r = _check_values(from_nhwc(Yc, cout), y64, bound, name)
    assert torch.all(Yc[..., cout:] == 0)
    be.check_all()
    print("%s mode %d plan %s ratio %.3g" % (name, bf16x3, got[5:], r))
