"""The kernels of csrc/predict.hip (the prediction task around its GRU): the window gather, the L1 loss fused with the output
head and its gradient, and the end of the roll-out, each against torch / float64 restatements of the reference's statements
(prediction.py:28-32,97-103,121-131; modules/prediction_module.py:33-42).  Every buffer is guard-banded and const arguments
are checked (tests/_guard.py); the same bodies run on the CPU emulator and, with -m gpu, on the MI355X."""
import pytest
import torch
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)

from test_predictor import head64


def rows_of(kp):
    """the predictor's input rows (prediction_module.py:28-33): all means, then all covariances"""
    b, t = kp["mean"].shape[:2]
    return torch.cat([kp[k].reshape(b, t, -1) for k in ("mean", "var") if k in kp], -1)


def l1_loss(gt, prediction, init_frames):
    """prediction.py:103"""
    return sum([torch.abs(gt[k][:, init_frames:] - prediction[k][:, init_frames:]).mean() for k in gt])


def make_case(B, T, K, has_var, seed):
    g = torch.Generator().manual_seed(seed)
    F = 6 if has_var else 2
    y = torch.randn(B, T, K * F, generator=g)
    gt = {"mean": torch.rand(B, T, K, 2, generator=g) * 2 - 1}
    if has_var:
        gt["var"] = torch.randn(B, T, K, 2, 2, generator=g)
    return y, gt, F


# ---- gather ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("init_frames", [1, 2, 4])
@pytest.mark.parametrize("I,pad", [(6, 1), (18, 3), (10, 2), (20, 4), (60, 8)])      # (20, 4), (60, 8): the float4 form
def test_window_gather_equals_indexing(be, I, pad, init_frames):
    """B = 3 windows of T = 5 rows: one starts at row 0, one ends on the pool's last row (a row too far would read the guard
    band: NaN / 3e38), rows are `pad` floats wider than I and the pad floats never reach the outputs"""
    B, T, R = 3, 5, 12
    g = torch.Generator().manual_seed(I + init_frames)
    pool = torch.randn(R, I + pad, generator=g)
    pool[:, I:] = 777.0
    starts = torch.tensor([0, R - T, 3], dtype=torch.int64)
    x, gt = be.empty(B, T, I), be.empty(B, T, I)
    be.call("mnk_kp_window_gather", be.t(pool), R, I + pad, be.t(starts), B, T, init_frames, I, x, gt)
    be.sync()
    ref = torch.stack([pool[s:s + T, :I] for s in starts.tolist()])
    x, gt = x.cpu(), gt.cpu()
    assert torch.equal(gt, ref)
    assert torch.equal(x[:, :init_frames], ref[:, :init_frames])
    assert (x[:, init_frames:] == 0.0).all() and not torch.signbit(x[:, init_frames:]).any()


def test_window_gather_row_outside_the_pool_is_nan(be):
    """a start past the pool reads nothing (the guard band of the pool would show as 3e38 / a tagged NaN pattern mix)"""
    B, T, I, R = 2, 3, 6, 4
    pool = torch.arange(R * I, dtype=torch.float32).view(R, I)
    x, gt = be.empty(B, T, I), be.empty(B, T, I)
    be.call("mnk_kp_window_gather", be.t(pool), R, I, be.t(torch.tensor([0, 2], dtype=torch.int64)), B, T, 1, I, x, gt)
    be.sync()
    gt = gt.cpu()
    assert torch.equal(gt[0], pool[:3]) and torch.equal(gt[1, :2], pool[2:])
    assert torch.isnan(gt[1, 2]).all()


# ---- L1 loss fused with the head --------------------------------------------------------------------------------------------------
SHAPES = [(3, 5, 3, 1), (3, 5, 5, 2), (2, 3, 1, 2), (37, 9, 10, 1)]


def fused(be, y, gt_rows, B, T, K, F, has_var, init_frames, acc=None, log=None):
    ws_n = be.query("mnk_gru_head_l1_workspace_floats", B, T, K)
    loss, dy, ws = be.empty(1), be.empty(B * T, K * F), be.empty(ws_n)
    yd, gd = be.t(y), be.t(gt_rows)
    be.call("mnk_gru_head_l1_fwd", yd, gd, B, T, K, F, int(has_var), init_frames, loss, acc, log, 0 if log is None else log.numel(),
            ws, ws_n)
    be.call("mnk_gru_head_l1_bwd", yd, gd, B, T, K, F, int(has_var), init_frames, dy)
    be.sync()
    return loss.cpu(), dy.cpu().view(B, T, K, F)


def references(be, y, gt, K, has_var, init_frames):
    """(loss64, dy64, |gt - p64| per key, loss of HeadFn + the stock fp32 loss on the backend's device, its dy)"""
    y64 = y.double().requires_grad_()
    out64 = head64(y64, K, has_var)
    gt64 = {k: v.double() for k, v in gt.items()}
    loss64 = l1_loss(gt64, out64, init_frames)
    loss64.backward()
    dist = {k: (gt64[k] - out64[k]).detach().abs() for k in gt}
    from mnk.gru import HeadFn
    y32 = y.to(be.device).requires_grad_()
    o = HeadFn.apply(y32, K, has_var)
    out32 = {"mean": o[0], "var": o[1]} if has_var else {"mean": o}
    loss32 = l1_loss({k: v.to(be.device) for k, v in gt.items()}, out32, init_frames)
    loss32.backward()
    be.sync()
    return float(loss64.detach()), y64.grad, dist, float(loss32.detach().double()), y32.grad.cpu()


def ambiguous_key_points(dist, init_frames, has_var):
    """(b, t, k) of the loss frames where some |gt - p64| < 1e-5: the sign there is the implementation's rounding"""
    near = (dist["mean"] < 1e-5).any(-1)
    if has_var:
        near = near | (dist["var"] < 1e-5).flatten(-2).any(-1)
    near[:, :init_frames] = False
    return near


@pytest.mark.parametrize("has_var", [True, False])
@pytest.mark.parametrize("B,T,K,init_frames", SHAPES)
def test_head_l1_against_fp64(be, B, T, K, init_frames, has_var):
    """odd element counts, one frame in the loss ((2, 3, 1, 2)), 3 330 key points = 14 blocks of partials ((37, 9, 10, 1)).
    The fused loss and gradient may be twice as far from float64 as HeadFn + the stock fp32 loss on the same inputs, plus the
    kernel tolerance 1e-6.  With these seeds the float64 reference has no element within 1e-5 of its
    ground truth (checked: the list of left-out key points is empty; at most two would be allowed)"""
    y, gt, F = make_case(B, T, K, has_var, 1000 * B + 10 * T + K + int(has_var))
    loss, dy = fused(be, y, rows_of(gt), B, T, K, F, has_var, init_frames)
    loss64, dy64, dist, loss32, dy32 = references(be, y, gt, K, has_var, init_frames)
    e_fused, e_unfused = abs(float(loss.double()) - loss64), abs(loss32 - loss64)
    print("loss: fused %.3e unfused32 %.3e of %.6f" % (e_fused, e_unfused, loss64))
    assert e_fused <= 2 * e_unfused + 1e-6 * abs(loss64)

    near = ambiguous_key_points(dist, init_frames, has_var)
    left_out = near.nonzero().tolist()
    print("left out:", left_out)
    assert len(left_out) <= 2
    keep = (~near)[..., None].expand(B, T, K, F)
    dy64 = dy64.view(B, T, K, F)
    scale = float(dy64.abs().max())
    # per tensor: the means' and the covariances' part of dy
    for name, sl in (("mean", slice(0, 2)), ("var", slice(2, 6))) if has_var else (("mean", slice(0, 2)),):
        k = keep[..., sl]
        e_f = float(((dy[..., sl].double() - dy64[..., sl]).abs() * k).max())
        e_u = float(((dy32.view(B, T, K, F)[..., sl].double() - dy64[..., sl]).abs() * k).max())
        print("dy %s: fused %.3e unfused32 %.3e of %.3e" % (name, e_f, e_u, scale))
        assert e_f <= 2 * e_u + 1e-6 * scale, name
    z = dy[:, :init_frames]
    assert (z == 0.0).all() and not torch.signbit(z).any()


@pytest.mark.parametrize("has_var", [True, False])
def test_head_l1_zero_gradient_where_gt_equals_the_prediction(be, has_var):
    """torch.abs' sign(0) = 0: elements whose ground truth IS the fp32 prediction (taken from mnk_gru_head_fwd, which shares
    the per-key-point functions) get gradient exactly 0; their neighbours do not"""
    B, T, K, init_frames = 3, 5, 3, 1
    y, gt, F = make_case(B, T, K, has_var, 77)
    mean, var = be.empty(B, T, K, 2), be.empty(B, T, K, 2, 2) if has_var else None
    be.call("mnk_gru_head_fwd", be.t(y), B * T, K, F, int(has_var), mean, var)
    be.sync()
    hits = [(0, 1, 0), (2, 4, 2), (1, 3, 1)]
    for b, t, k in hits:
        gt["mean"][b, t, k, 1] = mean.cpu()[b, t, k, 1]
        if has_var:
            gt["var"][b, t, k] = var.cpu()[b, t, k]
    _, dy = fused(be, y, rows_of(gt), B, T, K, F, has_var, init_frames)
    for b, t, k in hits:
        assert dy[b, t, k, 1] == 0.0 and dy[b, t, k, 0] != 0.0
        if has_var:
            assert (dy[b, t, k, 2:] == 0.0).all()
    assert int((dy[:, init_frames:] == 0.0).sum()) == len(hits) * (5 if has_var else 1)


def test_head_l1_is_deterministic_and_accumulates_in_order(be):
    """two calls: bit-identical loss and dy; the epoch accumulator holds (l + l, 2) and the log both losses"""
    B, T, K, init_frames = 37, 9, 10, 1
    y, gt, F = make_case(B, T, K, True, 5)
    acc, log = be.zeros(2), be.empty(3)
    l0, dy0 = fused(be, y, rows_of(gt), B, T, K, F, True, init_frames, acc, log)
    l1, dy1 = fused(be, y, rows_of(gt), B, T, K, F, True, init_frames, acc, log)
    assert torch.equal(l0, l1) and torch.equal(dy0, dy1)
    acc, log = acc.cpu(), log.cpu()
    assert float(acc[1]) == 2.0 and acc[0] == l0[0] + l0[0]
    assert torch.equal(log[:2], torch.cat([l0, l1])) and torch.isnan(log[2])


def test_head_l1_workspace_is_checked(be):
    """a workspace one float short of the query is refused (or not overrun)"""
    B, T, K = 37, 9, 10
    y, gt, F = make_case(B, T, K, True, 6)
    be.ws_shrink = 1
    fused(be, y, rows_of(gt), B, T, K, F, True, 1)
    assert [e[2] for e in be.ws_log if e[0] == "mnk_gru_head_l1_fwd"] == ["raised"]


# ---- the end of the roll-out --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_var", [True, False])
@pytest.mark.parametrize("predict_variance", [True, False])
@pytest.mark.parametrize("init_frames", [1, 3])
def test_rollout_finish_equals_the_reference_statements(be, init_frames, predict_variance, has_var):
    B, T, K = 2, 5, 3
    g = torch.Generator().manual_seed(init_frames + 2 * predict_variance)
    kp_init = {"mean": torch.randn(B, T, K, 2, generator=g)}
    kp_video = {"mean": torch.randn(B, T, K, 2, generator=g)}
    if has_var:
        kp_init["var"] = torch.randn(B, T, K, 2, 2, generator=g)
        kp_video["var"] = torch.randn(B, T, K, 2, 2, generator=g)
    for k in kp_init:                                   # prediction.py:121-122
        kp_init[k][:, init_frames:] = 0
    init_rows = rows_of(kp_init)
    I = init_rows.shape[-1]
    padded = torch.full((B * T, I + 2), 777.0)
    padded[:, :I] = init_rows.view(B * T, I)
    mean = be.t(kp_video["mean"])
    var = be.t(kp_video["var"]) if has_var else None
    be.call("mnk_kp_rollout_finish", be.t(padded), I + 2, B, T, K, int(has_var), init_frames, int(predict_variance), mean, var)
    be.sync()
    # prediction.py:127-131
    for k in kp_video:
        kp_video[k][:, :init_frames] = kp_init[k][:, :init_frames]
    if 'var' in kp_video and predict_variance:
        kp_video['var'] = kp_init['var'][:, (init_frames - 1):init_frames].repeat(1, kp_video['var'].shape[1], 1, 1, 1)
    assert torch.equal(mean.cpu(), kp_video["mean"])
    if has_var:
        assert torch.equal(var.cpu(), kp_video["var"])
