"""The row-tile grouped 1x1 kernels, the head weight gradient that finishes in its partial kernel, and the K x K packs that the
optimiser kernel emits: against float64 NumPy (tolerances of tests/test_kernels_motion.py: 1e-6 relative for outputs and data
gradients, 1e-5 for weight / bias gradients), pad channels exactly zero over a NaN pre-fill, guard bands around every buffer;
the packs bit for bit against the pack kernel."""
import numpy as np
import pytest
import torch

from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from _util import ceil4, relerr

MAXG = 8
ROWS = (1, 63, 257, 1030)


def _gconv_data(rows, G, S, ld, seed):
    rng = np.random.default_rng(seed)
    C = G * S
    x = np.zeros((rows, ld), dtype=np.float32)
    x[:, :C] = rng.standard_normal((rows, C), dtype=np.float32)
    w = rng.standard_normal((C, S), dtype=np.float32)
    b = rng.standard_normal(C, dtype=np.float32)
    return x, w, b


def _gconv_ref(x, w, b, G, S, transpose):
    """float64: y[r, g*S + o] = b + sum_k x[r, g*S + k] w[g*S + o, k]  (transpose: sum over o of x[r, g*S + o] w[g*S + o, k])"""
    rows = x.shape[0]
    xg = x[:, :G * S].astype(np.float64).reshape(rows, G, S)
    wg = w.astype(np.float64).reshape(G, S, S)
    y = np.einsum("rgo,gok->rgk", xg, wg) if transpose else np.einsum("rgk,gok->rgo", xg, wg)
    y = y.reshape(rows, G * S)
    return y + b.astype(np.float64) if b is not None else y


def _check_gconv_fwd(be, rows, G, S, ld_x, ld_y, transpose, bias, seed=0):
    C = G * S
    x, w, b = _gconv_data(rows, G, S, ld_x, seed)
    X, W, Bt = be.t(torch.from_numpy(x)), be.t(torch.from_numpy(w)), be.t(torch.from_numpy(b))
    Y = be.empty(rows, ld_y)                       # NaN: a pad channel that is not written shows
    if transpose:
        be.call("mnk_gconv1x1_bwd_data", X, ld_x, W, Y, ld_y, rows, G, S)
    else:
        be.call("mnk_gconv1x1_fwd", X, ld_x, W, Bt if bias else None, Y, ld_y, rows, G, S)
    be.sync()
    y = Y.cpu()
    ref = torch.from_numpy(_gconv_ref(x, w, b if (bias and not transpose) else None, G, S, transpose))
    tag = (rows, G, S, ld_x, ld_y, transpose, bias)
    assert relerr(y[:, :C], ref) < 1e-6, tag
    assert torch.equal(y[:, C:], torch.zeros(rows, ld_y - C)), tag


@pytest.mark.parametrize("S", [1, 2, 6, MAXG])
@pytest.mark.parametrize("G", [1, 3, 11])
def test_gconv1x1_forward_and_data_gradient(be, G, S):
    """rows that are no multiple of the tile or of 4, pitches with and without pad channels, both `transpose` values, with
    and without bias"""
    C = G * S
    for rows in ROWS:
        for pad in (0, 8):
            ld = ceil4(C) + pad
            _check_gconv_fwd(be, rows, G, S, ld, ld, 0, True)
            _check_gconv_fwd(be, rows, G, S, ld, ld, 0, False)
            _check_gconv_fwd(be, rows, G, S, ld, ld, 1, False)


@pytest.mark.parametrize("G,S,ld_x,ld_y", [
    (3, 6, 19, 21),          # pitches that are no multiple of 4: scalar staging and scalar row stores
    (11, 6, 68, 76),         # different pitches on the two sides
    (2048, 1, 2048, 2048),   # G * S * (S + 1) == 4096: the widest staged weights; 512 quads per row: a thread walks two
    (2049, 1, 2052, 2052),   # one group more: the thread-per-(row, group) kernel
    (56, 8, 448, 448),       # G * S * (S + 1) = 4032 <= 4096 with 8 x 8 groups
    (57, 8, 456, 460),       # 4104 > 4096: the thread-per-(row, group) kernel
    (1, 1, 4092, 8),         # the widest row pitch that fits the tile (one row per tile)
    (1, 1, 4093, 8),         # one float more: the thread-per-(row, group) kernel
])
def test_gconv1x1_forward_on_both_sides_of_the_staging_limits(be, G, S, ld_x, ld_y):
    for rows in (1, 5):
        _check_gconv_fwd(be, rows, G, S, ld_x, ld_y, 0, True)
        _check_gconv_fwd(be, rows, G, S, ld_x, ld_y, 1, False)


def _check_gconv_wgrad(be, rows, G, S, ld_x, ld_dy, with_bias=True):
    C = G * S
    x, _, _ = _gconv_data(rows, G, S, ld_x, 1)
    dy, _, _ = _gconv_data(rows, G, S, ld_dy, 2)
    X, DY = be.t(torch.from_numpy(x)), be.t(torch.from_numpy(dy))
    nws = be.query("mnk_gconv1x1_workspace_floats", rows, G, S)
    ws, DW, DB = be.empty(nws), be.empty(C, S), be.empty(C)
    be.call("mnk_gconv1x1_bwd_weight", X, ld_x, DY, ld_dy, DW, DB if with_bias else None, rows, G, S, ws, nws)
    be.sync()
    xg = x[:, :C].astype(np.float64).reshape(rows, G, S)
    dg = dy[:, :C].astype(np.float64).reshape(rows, G, S)
    tag = (rows, G, S, ld_x, ld_dy)
    assert relerr(DW.cpu(), torch.from_numpy(np.einsum("rgo,rgk->gok", dg, xg).reshape(C, S))) < 1e-5, tag
    if with_bias:
        assert relerr(DB.cpu(), torch.from_numpy(dg.sum(0).reshape(C))) < 1e-5, tag
    else:
        assert torch.isnan(DB).all(), tag


@pytest.mark.parametrize("S", [1, 2, 6, MAXG])
@pytest.mark.parametrize("G", [1, 3, 11])
def test_gconv1x1_weight_gradient(be, G, S):
    """the same shapes; 4100 rows = three row blocks of 1367 rows, the last one a row short, each lane of a block with five or six
    rows"""
    C = G * S
    for rows in ROWS + (4100,):
        for pad in (0, 8):
            ld = ceil4(C) + pad
            _check_gconv_wgrad(be, rows, G, S, ld, ld)
    _check_gconv_wgrad(be, 63, G, S, C + 1, C + 3)              # odd pitches: 4-byte loads
    _check_gconv_wgrad(be, 63, G, S, ceil4(C), ceil4(C) + 4, with_bias=False)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("cout", [1, 2, 4])
@pytest.mark.parametrize("rows_hw,cin,misalign", [
    ((9, 11), 70, 0),       # 99 rows: one row block -- the partial kernel writes dw / dbias itself; 70 + 1 columns: two 64-chunks
    ((9, 11), 13, 1),       # the same through the thread-per-pixel data gradient (a tensor that is not 16-byte aligned)
    ((18, 11), 70, 0),      # 198 rows: two row blocks of 99 -- partials + the final kernel
])
def test_head_weight_gradient_with_one_and_with_two_row_blocks(be, rows_hw, cin, misalign, cout, act):
    H, W = rows_hw
    rows, ld = H * W, ceil4(cin) + (4 if misalign else 0)
    rng = np.random.default_rng(3)
    x = np.zeros((rows, ld), dtype=np.float32)
    x[:, :cin] = rng.standard_normal((rows, cin), dtype=np.float32)
    w = (rng.standard_normal((cout, cin)) * 0.3).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    dout = rng.standard_normal((1, cout, 1, H, W)).astype(np.float32)
    Xb = be.empty(rows * ld + 4)
    X = Xb[misalign:misalign + rows * ld].view(rows, ld)
    X.copy_(torch.from_numpy(x))
    Wt, Bt, DO = be.t(torch.from_numpy(w)), be.t(torch.from_numpy(b)), be.t(torch.from_numpy(dout))
    OUT = be.empty(1, cout, 1, H, W)
    be.call("mnk_conv1x1_fwd", X, ld, cin, Wt, Bt, OUT, 1, 1, H, W, cout, act)
    nws = be.query("mnk_conv1x1_workspace_floats", rows, cin, cout)
    ws, DX, DW, DB = be.empty(nws), be.empty(rows, ld), be.empty(cout, cin), be.empty(cout)
    be.call("mnk_conv1x1_bwd", X, ld, cin, Wt, OUT, DO, DX, ld, DW, DB, 1, 1, H, W, cout, act, ws, nws)
    DW2 = be.empty(cout, cin)                     # parameters only, no bias gradient asked for
    be.call("mnk_conv1x1_bwd", X, ld, cin, Wt, OUT, DO, None, ld, DW2, None, 1, 1, H, W, cout, act, ws, nws)
    be.sync()
    pre = x[:, :cin].astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)          # [rows][cout]
    o = 1.0 / (1.0 + np.exp(-pre)) if act else pre
    d = dout.astype(np.float64).reshape(cout, rows).T
    dpre = d * o * (1.0 - o) if act else d
    assert float((OUT.cpu().double().reshape(cout, rows).T - torch.from_numpy(o)).abs().max()) < 1e-6
    assert relerr(DX.cpu()[:, :cin], torch.from_numpy(dpre @ w.astype(np.float64))) < 1e-5
    assert torch.equal(DX.cpu()[:, cin:], torch.zeros(rows, ld - cin))
    assert relerr(DW.cpu(), torch.from_numpy(dpre.T @ x[:, :cin].astype(np.float64))) < 1e-5
    assert relerr(DB.cpu(), torch.from_numpy(dpre.sum(0))) < 1e-5
    assert torch.equal(DW2.cpu(), DW.cpu())


# ---- the optimiser kernel writes the K x K packs ------------------------------------------------------------------------------
def _two_conv_model(be):
    """the discriminator's first convolution (4x4, 13 -> 64 channels) and a 3x3 convolution over two sources"""
    g = torch.Generator().manual_seed(5)
    w4 = torch.nn.Parameter(be.t(torch.randn(64, 13, 1, 4, 4, generator=g) * 0.1))
    w3 = torch.nn.Parameter(be.t(torch.randn(20, 9 + 5, 1, 3, 3, generator=g) * 0.1))
    return w4, w3


def _forward_backward(be, w4, w3):
    from mnk import ops
    g = torch.Generator().manual_seed(6)
    a = ops.to_act(be.t(torch.rand(2, 13, 1, 9, 9, generator=g))).requires_grad_(True)
    y4 = ops.ConvKxKFn.apply(a, w4, None, 13, 4, 4, 0, False)
    b0 = ops.to_act(be.t(torch.rand(2, 9, 1, 6, 6, generator=g))).requires_grad_(True)
    b1 = ops.to_act(be.t(torch.rand(2, 5, 1, 6, 6, generator=g))).requires_grad_(True)
    y3, _ = ops.conv3x3(b0, 9, w3, x1=b1, c1=5)
    ((y4 * y4).sum() + (y3 * y3).sum()).backward()


def _assert_packs_are_those_of_the_pack_kernel(be, w4, w3):
    from mnk import ops
    be.sync()
    e4, e3 = ops.pack_entry_of(w4), ops.pack_entry_of(w3)
    assert e4 is not None and e4.ntaps == 16 and e4.wd[0] is not None
    assert e3 is not None and e3.ntaps == 9 and e3.wd[0] is not None and e3.wd[1] is not None
    f4, d4 = torch.full_like(e4.wp, float("nan")), torch.full_like(e4.wd[0], float("nan"))
    be.call("mnk_conv2d_pack_all", w4.detach(), f4, d4, None, 64, 13, 0, 16)
    f3, d30, d31 = (torch.full_like(t, float("nan")) for t in (e3.wp, e3.wd[0], e3.wd[1]))
    be.call("mnk_conv3x3_pack_all", w3.detach(), f3, d30, d31, 20, 9, 5)
    be.sync()
    for name, mine, ref in (("4x4 forward", e4.wp, f4), ("4x4 data gradient", e4.wd[0], d4), ("3x3 forward", e3.wp, f3),
                            ("3x3 data gradient, source 0", e3.wd[0], d30), ("3x3 data gradient, source 1", e3.wd[1], d31)):
        assert torch.equal(mine, ref), name


def _count_launches(fn):
    from mnk import ops
    names, real = [], ops._call

    def counting(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    ops._call = counting
    try:
        fn()
    finally:
        ops._call = real
    return names


def test_mnk_adam_writes_the_4x4_packs_of_the_updated_weights(be):
    from mnk import ops, optim as moptim
    w4, w3 = _two_conv_model(be)
    opt = moptim.MnkAdam([w4, w3], lr=1e-2, betas=(0.5, 0.999))
    _forward_backward(be, w4, w3)                 # first use: per-layer packs register both weights
    before = w4.detach().clone()
    opt.step()
    be.sync()
    assert not torch.equal(before, w4.detach())
    _assert_packs_are_those_of_the_pack_kernel(be, w4, w3)
    assert ops.repack_registered(only_if_stale=True) is False           # nothing stale
    opt.zero_grad()
    names = _count_launches(lambda: _forward_backward(be, w4, w3))
    assert not [n for n in names if "pack" in n], names
    # a write from outside: stale again, and every registered K x K weight (this one, and whatever else the process still
    # holds) goes through the pack kernel once more, the 3x3 ones in their one launch
    w4.data.mul_(0.5)
    ops.invalidate_packed_weights()
    names = _count_launches(lambda: ops.repack_registered(only_if_stale=True))
    kxk = sum(1 for e in ops._PACK_REG.values() if e.ntaps != 9 and e.wref() is not None)
    assert kxk >= 1 and names.count("mnk_conv2d_pack_all") == kxk and names.count("mnk_conv3x3_pack_multi") == 1, names
    _assert_packs_are_those_of_the_pack_kernel(be, w4, w3)


def test_adopted_adam_writes_the_4x4_packs_of_the_updated_weights(be):
    from mnk import ops, optim as moptim
    w4, w3 = _two_conv_model(be)
    opt = torch.optim.Adam([w4, w3], lr=1e-2, betas=(0.5, 0.999))
    sinks = moptim.GradSinks([w4, w3])
    moptim.install_adam_adoption()
    _forward_backward(be, w4, w3)
    before = w4.detach().clone()
    opt.step()
    be.sync()
    assert moptim.adopted(opt) is not None and moptim.adopted(opt).steps_taken == 1
    assert not torch.equal(before, w4.detach())
    _assert_packs_are_those_of_the_pack_kernel(be, w4, w3)
    assert ops.repack_registered(only_if_stale=True) is False
    del sinks


def test_second_training_iteration_has_no_pack_launch(be):
    """two eager TrainStep iterations of the tiny configuration: the optimiser kernels of the first leave every packed layout
    (3x3, sub-pixel and the discriminator's 4x4) ready for the second"""
    from mnk import engine
    from oracle import cases
    from test_modules import build
    cfg = cases.TINY
    gen, disc, kpd = build(cfg)
    gen.to(be.device), disc.to(be.device), kpd.to(be.device)
    step = engine.TrainStep(gen, disc, kpd, cfg["train_params"], fused_adam=True, use_graph=False)
    src, drv = cases.smooth_pair(2, 32, 32)
    x = {"source": be.t(src), "video": be.t(drv)}
    first = _count_launches(lambda: step.step(x))
    second = _count_launches(lambda: step.step(x))
    be.sync()
    assert [n for n in first if "pack" in n], "the first iteration packs per layer"
    assert not [n for n in second if "pack" in n], [n for n in second if "pack" in n]
    # parameters written from outside: the next iteration re-packs through the pack kernels
    step.weights_changed()
    third = _count_launches(lambda: step.step(x))
    assert "mnk_conv3x3_pack_multi" in third and "mnk_conv2d_pack_all" in third
