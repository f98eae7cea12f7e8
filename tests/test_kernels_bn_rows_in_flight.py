"""The first-stage norm kernels with several rows of a thread's walk in flight (csrc/batchnorm.hip: walk_rows) through their C
entry points, on guard-banded buffers whose guards and unwritten parts are NaN: a row past a thread's range that is loaded AND
used shows up in a sum or an output.  Reference: an fp64 restatement of the formulas below, at test_kernels_bn.py's tolerances
(z: 2e-5 absolute; sums and dy: 1e-4 relative; column sums of dy: 1e-5 of the largest absolute column sum + 1e-6).

The thread map (make_map) is restated here so that the shapes hit the loop's cases: with `tx` = channel quads and `ty` = 256 // tx
row lanes per block, a block of P rows gives every thread P // ty or P // ty + 1 rows; the tuning values bn_rpt / bn_blocks (sums
and backward apply) and bn_fwd_rpt / bn_fwd_blocks (forward apply) are set so that small tensors are cut into three row blocks
of P rows, the last one two rows short."""
import ctypes

import pytest
import torch

from _util import ceil4, relerr, maxerr
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)

NAN = float("nan")
_KNOBS = (b"bn_rpt", b"bn_blocks", b"bn_fwd_rpt", b"bn_fwd_blocks")


class _Map:
    """bn_rpt = bn_fwd_rpt = rpt, bn_blocks = bn_fwd_blocks = blocks while the block runs"""

    def __init__(self, be, rpt, blocks):
        self.be, self.want = be, (rpt, blocks, rpt, blocks)

    def __enter__(self):
        self.old = []
        for name, v in zip(_KNOBS, self.want):
            o = ctypes.c_int(0)
            self.be.lib.call("mnk_get_tuning", name, ctypes.byref(o))
            self.old.append(o.value)
            self.be.lib.call("mnk_set_tuning", name, v)

    def __exit__(self, *exc):
        for name, v in zip(_KNOBS, self.old):
            self.be.lib.call("mnk_set_tuning", name, v)


def _ty(c):
    nv = ceil4(c) // 4
    assert nv <= 64
    return 256 // nv


# ---- fp64 restatement (NHWC, channels last) -------------------------------------------------------------------------------------
def _act(v, slope):
    return v if slope < 0 else torch.where(v > 0, v, v * slope)


def _per_row(p, n, h, w, per_frame):
    """a parameter vector ((n *) c) as (n, 1, 1, c) / (1, 1, 1, c)"""
    return p.double().view(n, 1, 1, -1) if per_frame else p.double().view(1, 1, 1, -1)


def ref_fwd(y, mean, scale, beta, slope, pool, per_frame):
    n, h, w, c = y.shape
    z = _act((y.double() - _per_row(mean, n, h, w, per_frame)) * _per_row(scale, n, h, w, per_frame) + beta.double(), slope)
    if pool:
        ho, wo = h // 2, w // 2
        z = z[:, :2 * ho, :2 * wo].reshape(n, ho, 2, wo, 2, c).sum((2, 4)) * 0.25
    return z


def ref_bwd(y, dz, mean, invstd, scale, beta, slope, pool, per_frame, count, training, addend=None):
    """(sums [2, frames, c], dy)"""
    n, h, w, c = y.shape
    m, isd, sc = (_per_row(p, n, h, w, per_frame) for p in (mean, invstd, scale))
    d = y.double() - m
    if pool:
        ho, wo = h // 2, w // 2
        g = torch.zeros(n, h, w, c, dtype=torch.float64)
        g[:, :2 * ho, :2 * wo] = dz.double().repeat_interleave(2, 1).repeat_interleave(2, 2) * 0.25
    else:
        g = dz.double().clone()
    if slope >= 0:
        g = torch.where(d * sc + beta.double() > 0, g, g * slope)
    xh = d * isd
    dims = (1, 2) if per_frame else (0, 1, 2)
    s1, s2 = g.sum(dims, keepdim=True), (g * xh).sum(dims, keepdim=True)
    dy = sc * (g - s1 / count - xh * s2 / count) if training else sc * g
    if addend is not None:
        dy = dy + addend.double()
    frames = n if per_frame else 1
    return torch.stack([s1.reshape(frames, c), s2.reshape(frames, c)]), dy


# ---- one layer through every entry point ----------------------------------------------------------------------------------------
def _strided(be, x, ld, off=0, fill=NAN):
    """x (..., c) as a device buffer (..., ld) with x at channel `off` and `fill` elsewhere"""
    out = torch.full(x.shape[:-1] + (ld,), fill)
    out[..., off:off + x.shape[-1]] = x
    return be.t(out)


def run_layer(be, n, h, w, c, *, slope=0.0, pool=0, per_frame=0, training=1, dz_off=0, ld_dz=None, addend=False, seed=0,
              ld_x_extra=0):
    """stats, forward apply, backward sums, backward apply (plain, and for BatchNorm with ReLU / no activation the _colsum and
    _add_colsum forms) of one layer against the restatement"""
    g = torch.Generator().manual_seed(1000 * c + 10 * h + w + seed)
    ldc = ceil4(c)
    frames = n if per_frame else 1
    y = torch.randn(n, h, w, c, generator=g) * 1.5 + 0.3
    mean = torch.randn(frames * c, generator=g) * 0.3
    invstd = torch.rand(frames * c, generator=g) + 0.5
    gamma = torch.rand(c, generator=g) + 0.5
    scale = (invstd.view(frames, c) * gamma).reshape(-1)
    beta = torch.randn(c, generator=g) * 0.3
    ho, wo = (h // 2, w // 2) if pool else (h, w)
    dz = torch.randn(n, ho, wo, c, generator=g)
    skip = torch.randn(n, h, w, c, generator=g)
    rows = n * h * w
    count = float(h * w if per_frame else rows)
    Y = _strided(be, y, ldc, fill=0.0)
    MEAN, INV, SC, BT = be.t(mean), be.t(invstd), be.t(scale), be.t(beta)

    # forward statistics: sum x, sum x^2 (ld > round_up(C, 4): the pad quads are walked too and hold finite values)
    ldx = ldc + ld_x_extra
    X = _strided(be, y, ldx, fill=0.5)
    nws = be.query("mnk_norm_workspace_floats", h * w if per_frame else rows, frames, ldx)
    ws, sums = be.empty(nws), be.empty(2 * frames * c)
    be.call("mnk_norm_stats", X, ldx, h * w if per_frame else rows, frames, c, sums, ws, nws)
    dims = (1, 2) if per_frame else (0, 1, 2)
    want = torch.stack([y.double().sum(dims).reshape(frames, c), (y.double() ** 2).sum(dims).reshape(frames, c)])
    assert relerr(sums.cpu().view(2, frames, c), want) < 1e-4

    # forward apply: into a plain act (owns its pad channels) and into channels 4 ... of a wider one
    zr = ref_fwd(y, mean, scale, beta, slope, pool, per_frame)
    for ldz, zoff in ((ldc, 0), (ldc + 8, 4), (ldc + 7, 3)):
        Z = be.empty(n, ho, wo, ldz)
        be.call("mnk_norm_act_fwd", Y, ldc, MEAN, SC, BT, per_frame, Z, ldz, zoff, n, h, w, c, slope, pool)
        zc = Z.cpu()
        assert maxerr(zc[..., zoff:zoff + c], zr) < 2e-5
        if zoff == 0:
            assert torch.all(zc[..., c:] == 0)
        else:
            assert torch.all(torch.isnan(zc[..., :zoff])) and torch.all(torch.isnan(zc[..., zoff + c:]))

    # backward
    ld_dz = ld_dz or ldc + dz_off
    DZ = _strided(be, dz, ld_dz, dz_off)
    sr, dyr = ref_bwd(y, dz, mean, invstd, scale, beta, slope, pool, per_frame, count, training)
    nws = be.query("mnk_norm_workspace_floats", h * w if per_frame else rows, frames, ldc)
    ws, bs = be.empty(nws), be.empty(2 * frames * c)
    be.call("mnk_norm_act_bwd_stats", Y, ldc, DZ, ld_dz, dz_off, MEAN, INV, SC, BT, per_frame, n, h, w, c, slope, pool, bs, ws, nws)
    assert relerr(bs.cpu().view(2, frames, c), sr) < 1e-4
    BS = be.t(sr.float().reshape(-1))          # the apply pass is checked on the reference's sums
    DY = be.empty(n, h, w, ldc)
    be.call("mnk_norm_act_bwd_apply", Y, ldc, DZ, ld_dz, dz_off, MEAN, INV, SC, BT, per_frame, BS if training else None, count,
            training, DY, ldc, n, h, w, c, slope, pool)
    dyc = DY.cpu()
    assert relerr(dyc[..., :c], dyr) < 1e-4 and torch.all(dyc[..., c:] == 0)
    if per_frame or slope > 0:
        return
    relu = 1 if slope == 0 else 0
    nws = be.query("mnk_bn_workspace_floats", rows, ldc)
    DY2, dys = be.empty(n, h, w, ldc), be.empty(c)
    be.call("mnk_bn_act_bwd_apply_colsum", Y, ldc, DZ, ld_dz, dz_off, MEAN, INV, SC, BT, BS if training else None, count, training,
            DY2, ldc, n, h, w, c, relu, pool, dys, be.empty(nws), nws)
    d2 = DY2.cpu()
    assert torch.equal(d2, dyc)
    col = d2.double().reshape(-1, ldc)
    assert maxerr(dys.cpu(), col.sum(0)[:c]) <= 1e-5 * float(col.abs().sum(0).max()) + 1e-6
    if addend:
        lda = ldc + 4
        ADD = _strided(be, skip, lda)
        ADD[..., c:ldc] = 0
        DY3, dys3 = be.empty(n, h, w, ldc), be.empty(c)
        be.call("mnk_bn_act_bwd_apply_add_colsum", Y, ldc, DZ, ld_dz, dz_off, MEAN, INV, SC, BT, BS if training else None, count,
                training, ADD, lda, DY3, ldc, n, h, w, c, relu, pool, dys3, be.empty(nws), nws)
        d3 = DY3.cpu()
        assert relerr(d3[..., :c], dyr + skip.double()) < 1e-4 and torch.all(d3[..., c:] == 0)
        col = d3.double().reshape(-1, ldc)
        assert maxerr(dys3.cpu(), col.sum(0)[:c]) <= 1e-5 * float(col.abs().sum(0).max()) + 1e-6


# rows of a block = P: one, three (+ one row), four, five (- one row) and nine rows per thread -- a last batch shorter than, as
# long as and longer than a full one, with and without full batches in front
_BLOCK_ROWS = {"1": lambda ty: ty, "3+": lambda ty: 3 * ty + 1, "4": lambda ty: 4 * ty, "5-": lambda ty: 5 * ty - 1,
               "9": lambda ty: 9 * ty}


@pytest.mark.parametrize("per_thread", list(_BLOCK_ROWS))
@pytest.mark.parametrize("c", [3, 10, 13, 45, 64])
def test_rows_per_thread(be, c, per_thread):
    """Three row blocks of P rows, the last one two rows short; pad lanes (C = 3, 10, 13, 45), tx not dividing 256 (C = 10, 45),
    ld > C in the statistics (walked pad quads)."""
    p = _BLOCK_ROWS[per_thread](_ty(c))
    rows = 3 * p - 2
    with _Map(be, 1, 3):
        run_layer(be, 1, 1, rows, c, addend=True, ld_x_extra=4 if c in (10, 64) else 0)


@pytest.mark.parametrize("shape", [(3, 12, 14), (3, 13, 12), (3, 12, 13)])
@pytest.mark.parametrize("c,blocks", [(10, 1), (45, 2)])
def test_pooled(be, shape, c, blocks):
    """(1,2,2) average pool behind the layer: even sizes, an odd height, an odd width (the last row / column is not pooled: its
    dz factor is 0); three to six rows per thread"""
    n, h, w = shape
    with _Map(be, 1, blocks):
        run_layer(be, n, h, w, c, pool=1, addend=True)
        run_layer(be, n, h, w, c, pool=1, dz_off=3, seed=1, addend=True)


@pytest.mark.parametrize("hw,c", [(2, 10), (2, 256), (5, 10), (5, 64)])
@pytest.mark.parametrize("pool", [0, 1])
def test_per_frame_statistics(be, hw, c, pool):
    """InstanceNorm + LeakyReLU(0.2): frames of 4 and 25 rows, N = 6 -- the rows of one thread (ty apart) lie in other frames,
    so a batch straddles two or three frames (C = 256: ty = 4, six rows per thread over the 2 x 2 frames; C = 64: nine over 5 x 5)"""
    with _Map(be, 1, 1):
        run_layer(be, 6, hw, hw, c, slope=0.2, pool=pool, per_frame=1)
        run_layer(be, 6, hw, hw, c, slope=0.2, pool=pool, per_frame=1, training=0, seed=1)


@pytest.mark.parametrize("dz_off,ld_extra", [(0, 0), (4, 4), (3, 5), (0, 1), (4, 3)])
@pytest.mark.parametrize("c", [10, 13, 45])
def test_dz_alignment(be, c, dz_off, ld_extra):
    """dz inside a wider act: quad reads (dz_off and ld_dz multiples of four; the last quad reaches into the NaN behind the
    layer's channels and drops it) and lane-by-lane reads (dz_off = 3, or ld_dz no multiple of four)"""
    ty = _ty(c)
    with _Map(be, 1, 2):
        run_layer(be, 1, 1, 2 * (5 * ty - 1) - 1, c, dz_off=dz_off, ld_dz=ceil4(c) + dz_off + ld_extra, addend=True)


@pytest.mark.parametrize("slope", [-1.0, 0.0, 0.2])
@pytest.mark.parametrize("training", [0, 1])
def test_activation_and_evaluation_mode(be, slope, training):
    """no activation, ReLU, LeakyReLU; evaluation mode (training = 0: dy = scale * g, no sums read)"""
    c = 13
    with _Map(be, 1, 2):
        run_layer(be, 2, 5, 2 * _ty(c) + 3, c, slope=slope, training=training, addend=True)
