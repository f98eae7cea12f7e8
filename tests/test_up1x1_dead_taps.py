"""Up-sampled convolutions on a 1 x 1 low-resolution source (tuning value up1x1_dead_taps; csrc/pack_tile.h: up1x1_live*).

Twelve of the 16 pseudo taps of the sub-pixel forms only ever meet padding there.  With the tuning value on, the weight-gradient
GEMM makes no tiles for them (their slices of the partials stay unwritten), every reader of those partials takes +0.f for them
without a load, and the optimiser kernel leaves the dead slices of the packs alone.  Everything here is bit for bit against the
same build with up1x1_dead_taps = 0, which keeps all 16 taps everywhere.

The kernel tests use ONE layer: N = 3, C0 = 20, C1 = 5 (two sources, ragged), Cout = 24; "wgrad_tap" = 2 and "wtap_minc" = 1 put
both sources of this narrow layer on the sub-pixel form (the default plan keeps it for layers wider than a 64-channel tile)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

from _util import to_nhwc
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from test_kernels_optim import ADAM_DESC, JOB, REDUCE_DESC, Plan, _table

N, C0, C1, COUT = 3, 20, 5, 24
CIN = C0 + C1
SENTINEL_BITS = 0x7FC12345                       # a tagged quiet NaN: what an unwritten float of a partial buffer must still hold
MARKER = 123.0                                   # the finite value the packs are pre-filled with
SOURCES = ((0, C0), (C0, C1))                    # (c_start, channels)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _sentinel(*shape):
    return torch.from_numpy(np.full(shape, SENTINEL_BITS, dtype=np.uint32).view(np.float32))


def _is_sentinel(t):
    return bool((_bits(t) == np.int32(SENTINEL_BITS)).all())


@contextlib.contextmanager
def tuning(lib, **values):
    """set tuning values of the library for the block and put the former ones back"""
    old = {}
    try:
        for k, v in values.items():
            cur = ctypes.c_int(0)
            lib.call("mnk_get_tuning", k.encode(), ctypes.addressof(cur))
            old[k] = cur.value
            lib.call("mnk_set_tuning", k.encode(), int(v))
        yield
    finally:
        for k, v in old.items():
            lib.call("mnk_set_tuning", k.encode(), v)


def subpixel_form(be, knob):
    return tuning(be.lib, wgrad_tap=2, wtap_minc=1, up1x1_dead_taps=knob)


def _live(be, dgrad=0):
    mask = be.query("mnk_up1x1_live_mask", dgrad)
    return [t for t in range(16) if (mask >> t) & 1]


def _axis_live(length, a, u):
    """forward / weight gradient: pseudo tap (a, u) of an axis reads low-resolution entry i + a - 1 + u -- inside for some i?"""
    return any(0 <= i + a - 1 + u < length for i in range(length))


def _axis_live_dgrad(length, t):
    """data gradient (4x4, stride 2, pad 1 over 2 * length entries of dy): tap t of an axis reads dy entry 2 i + t - 1"""
    return any(0 <= 2 * i + t - 1 < 2 * length for i in range(length))


def _inputs(hs, ws, n=N, seed=5):
    g = torch.Generator().manual_seed(seed + 16 * hs + ws)
    return (torch.randn(n, C0, hs, ws, generator=g), torch.randn(n, C1, hs, ws, generator=g),
            torch.randn(n, COUT, 2 * hs, 2 * ws, generator=g))


def _wgrad_partials(be, hs, ws, path):
    """the deferred partials of both sources, [(splits, 16, COUT, c) tensor on the CPU], from buffers pre-filled with the sentinel
    (guard bands: _guard.GuardedBackend checks them around every call and at teardown)"""
    x0, x1, dy = _inputs(hs, ws)
    DY = be.t(to_nhwc(dy))
    X = [be.t(to_nhwc(x0)), be.t(to_nhwc(x1))]
    ho, wo = 2 * hs, 2 * ws
    out = []
    if path == "single":
        for (c_start, c), Xs in zip(SOURCES, X):
            plan = Plan()
            assert be.query("mnk_conv2d_wgrad_plan2", N, ho, wo, c, COUT, 3, 3, 1, Xs.shape[-1], 1 | 2, ctypes.byref(plan)) == 0
            assert plan.layout == 2 and plan.splits >= 1 and plan.part_floats == plan.splits * 16 * COUT * c
            part = be.t(_sentinel(plan.part_floats))
            DW = be.empty(COUT, CIN, 3, 3)
            be.call("mnk_conv2d_wgrad", Xs, Xs.shape[-1], c, 1 | 2 | 4, ho, wo, 3, 3, 1, DY, DY.shape[-1], COUT, DW, CIN, c_start, N,
                    ho, wo, part, plan.part_floats)
            be.sync()
            out.append(part.cpu().view(plan.splits, 16, COUT, c))
        return out
    jobs = np.array([(Xs.data_ptr(), DY.data_ptr(), 0, 0, Xs.shape[-1], c, 1 | 2, DY.shape[-1], COUT, N, ho, wo, ho, wo, 3, 3, 1,
                      0, 0, 0) for (_, c), Xs in zip(SOURCES, X)], dtype=JOB)
    assert be.query("mnk_wgrad_grouped_plan", jobs.ctypes.data, len(jobs)) == 0
    assert all(int(v) % 4 == 3 for v in jobs["variant"]) and all(int(v) == 2 for v in jobs["layout"]), jobs
    parts = [be.t(_sentinel(int(f))) for f in jobs["part_floats"]]
    for k, p in enumerate(parts):
        jobs["part"][k] = p.data_ptr()
    nbytes = be.query("mnk_wgrad_grouped_table_bytes", len(jobs))
    host = torch.zeros(nbytes, dtype=torch.uint8)
    assert be.query("mnk_wgrad_grouped_build", jobs.ctypes.data, len(jobs), host.data_ptr(), nbytes) == 0
    dev = be.t(host)
    be.call("mnk_wgrad_grouped_launch", dev, host.data_ptr())
    be.sync()
    be.check_all("after the grouped launch")
    return [p.cpu().view(int(s), 16, COUT, c) for p, s, (_, c) in zip(parts, jobs["splits"], SOURCES)]


PATHS = ["single", "grouped"]


def test_the_live_sets_are_what_the_padding_rule_gives(be):
    """the helper's two sets, re-derived here from the rule every loader applies per axis (0 <= entry < length)"""
    fwd = [4 * (2 * a + b) + 2 * u + v for a in (0, 1) for b in (0, 1) for u in (0, 1) for v in (0, 1)
           if 0 <= 0 + a - 1 + u < 1 and 0 <= 0 + b - 1 + v < 1]               # low-resolution entry i + a - 1 + u, i = 0, of 1
    dgrad = [4 * ty + tx for ty in range(4) for tx in range(4)
             if 0 <= 2 * 0 + ty - 1 < 2 and 0 <= 2 * 0 + tx - 1 < 2]           # dy entry 2 i + ty - 1, i = 0, of 2
    assert _live(be, 0) == sorted(fwd) and len(fwd) == 4
    assert _live(be, 1) == sorted(dgrad) and len(dgrad) == 4
    with subpixel_form(be, 1):
        assert be.query("mnk_up1x1_dead_taps", N, 1, 1) == 1
        assert [be.query("mnk_up1x1_dead_taps", N, h, w) for h, w in ((2, 2), (1, 2), (2, 1))] == [0, 0, 0]
    with subpixel_form(be, 0):
        assert be.query("mnk_up1x1_dead_taps", N, 1, 1) == 0


@pytest.mark.parametrize("path", PATHS)
def test_parent_path_partials_are_zero_exactly_outside_the_live_set(be, path):
    """knob 0 on a 1 x 1 source: the weight-gradient GEMM writes all 16 slices, and the ones outside the helper's live set are
    exact +0.f (the live ones are not) -- the derivation of the live set from the loader itself"""
    live = _live(be)
    with subpixel_form(be, 0):
        parts = _wgrad_partials(be, 1, 1, path)
    for p in parts:
        for t in range(16):
            if t in live:
                assert bool((p[:, t] != 0).any()) and bool(torch.isfinite(p[:, t]).all()), t
            else:
                assert bool((_bits(p[:, t]) == 0).all()), t


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("hs,ws", [(2, 2), (1, 2), (2, 1)])
def test_other_sources_use_all_16_slices_and_ignore_the_knob(be, hs, ws, path):
    """2 x 2, 1 x 2 and 2 x 1 sources: the knob changes no bit, and all 16 slices are written (no float of the sentinel is left).
    On 2 x 2 every slice is non-zero; a 1 x W or H x 1 source has eight pseudo taps whose one-entry axis is outside -- written as
    zeros, and kept: only the square 1 x 1 source is in scope."""
    with subpixel_form(be, 0):
        base = _wgrad_partials(be, hs, ws, path)
    with subpixel_form(be, 1):
        got = _wgrad_partials(be, hs, ws, path)
    for p, q in zip(base, got):
        assert torch.equal(_bits(p), _bits(q))
        assert bool(torch.isfinite(p).all())                 # (the sentinel is a NaN)
        nonzero = [t for t in range(16) if bool((p[:, t] != 0).any())]
        assert nonzero == [t for t in range(16) if _axis_live(hs, (t >> 3) & 1, (t >> 1) & 1) and _axis_live(ws, (t >> 2) & 1, t & 1)]
        assert len(nonzero) == (16 if hs == ws == 2 else 8)


@pytest.mark.parametrize("path", PATHS)
def test_weight_gradient_leaves_the_dead_slices_unwritten(be, path):
    """knob 1: live slices bit-equal to knob 0, dead slices still the sentinel (guard bands: checked by the backend)"""
    live = _live(be)
    with subpixel_form(be, 0):
        base = _wgrad_partials(be, 1, 1, path)
    with subpixel_form(be, 1):
        got = _wgrad_partials(be, 1, 1, path)
    for p, q in zip(base, got):
        assert p.shape == q.shape
        for t in range(16):
            if t in live:
                assert torch.equal(_bits(p[:, t]), _bits(q[:, t])), t
            else:
                assert _is_sentinel(q[:, t]), t


@pytest.mark.parametrize("frames", [N, 1920], ids=["one-stage", "group-sums"])
def test_single_layer_entry_reduces_without_the_dead_slices(be, frames):
    """mnk_conv2d_wgrad without MNK_WGRAD_DEFER: its own reduction (conv3x3_wgrad_tap_reduce_kernel; 1920 frames: more than 12
    splits, so the group sums in front of it too) on a sentinel-filled workspace gives knob 0's gradient to the bit"""
    x0, x1, dy = _inputs(1, 1, n=frames)
    DY = be.t(to_nhwc(dy))
    res = []
    for knob in (0, 1):
        with subpixel_form(be, knob):
            DW = be.empty(COUT, CIN, 3, 3)
            for (c_start, c), src in zip(SOURCES, (x0, x1)):
                X = be.t(to_nhwc(src))
                plan = Plan()
                assert be.query("mnk_conv2d_wgrad_plan2", frames, 2, 2, c, COUT, 3, 3, 1, X.shape[-1], 1 | 2, ctypes.byref(plan)) == 0
                assert plan.layout == 2 and (plan.splits > 12) == (frames > N), plan.splits
                nws = be.query("mnk_conv3x3_up_wgrad_workspace_floats", frames, 2, 2, c, COUT)
                ws = be.t(_sentinel(nws))
                be.call("mnk_conv2d_wgrad", X, X.shape[-1], c, 1 | 2, 2, 2, 3, 3, 1, DY, DY.shape[-1], COUT, DW, CIN, c_start, frames,
                        2, 2, ws, nws)
            be.sync()
            res.append(DW.cpu())
    assert bool(torch.isfinite(res[0]).all()) and torch.equal(_bits(res[0]), _bits(res[1]))


def _synthetic_partials(splits, c, live, seed):
    """(zero-dead, sentinel-dead) partials (splits, 16, COUT, c) with the same random live slices"""
    g = torch.Generator().manual_seed(seed)
    zero = torch.zeros(splits, 16, COUT, c)
    sent = _sentinel(splits, 16, COUT, c).clone()
    for t in live:
        v = torch.randn(splits, COUT, c, generator=g)
        zero[:, t], sent[:, t] = v, v
    return zero, sent


@pytest.mark.parametrize("vec", [1, 0], ids=["vector-maps", "tile-maps"])
def test_reduce_kernels_never_load_the_dead_slices(be, vec):
    """mnk_wgrad_reduce_multi, layout 2, every thread map (flat: splits < 4 and C % 4 == 0; vector tap-major with 1 and 16 groups
    / the tile map: ragged C, many splits): sentinel-filled dead slices + MNK_REDUCE_UP1X1 == zero-filled ones without the bit"""
    live = _live(be)
    cases = [(1, 0), (2, 0), (1, 1), (2, 1), (5, 0), (5, 1), (40, 1), (40, 0)]        # (splits, source)
    rows, keep, blocks = [], [], 0
    for k, (splits, si) in enumerate(cases):
        c_start, c = SOURCES[si]
        zero, sent = _synthetic_partials(splits, c, live, 40 + k)
        for part, flag in ((zero, 0), (sent, 1)):
            P, DW = be.t(part), be.empty(COUT, CIN, 9)
            rows.append((P.data_ptr(), DW.data_ptr(), 2, splits, 9, COUT, c, CIN, c_start, 0, blocks, flag))
            blocks += be.query("mnk_wgrad_reduce_blocks", splits, COUT, c)
            keep.append((P, DW, c_start, c))
    with tuning(be.lib, wgrad_reduce_vec=vec):
        maps = {be.query("mnk_wgrad_reduce_map", 2, s, 9, COUT, SOURCES[si][1]) for s, si in cases}
        assert maps == ({0, 1, 2} if vec else {0, 1}), maps
        be.call("mnk_wgrad_reduce_multi", _table(be, np.array(rows, dtype=REDUCE_DESC)), len(rows), blocks)
        be.sync()
    for k in range(0, len(keep), 2):
        (_, A, c_start, c), (_, B, _, _) = keep[k], keep[k + 1]
        a, b = A.cpu()[:, c_start:c_start + c], B.cpu()[:, c_start:c_start + c]
        assert bool(torch.isfinite(a).all()) and bool((a != 0).any()), cases[k // 2]
        assert torch.equal(_bits(a), _bits(b)), cases[k // 2]


def _pack_views(wf, w0, w1):
    chunks = (16 * ((C0 + 15) // 16) + 16 * ((C1 + 15) // 16)) // 16
    dchunks = (COUT + 15) // 16
    assert wf.numel() == 4 * COUT * chunks * 4 * 16 and w0.numel() == C0 * dchunks * 256 and w1.numel() == C1 * dchunks * 256
    # forward [phase][co][chunk][tap4][16] -> pseudo tap 4 * phase + tap4; data gradient [ci][chunk][tap16][16]
    f = wf.cpu().view(4, COUT, chunks, 4, 16).permute(0, 3, 1, 2, 4).reshape(16, -1)
    return f, w0.cpu().view(C0, dchunks, 16, 16).permute(2, 0, 1, 3).reshape(16, -1), \
        w1.cpu().view(C1, dchunks, 16, 16).permute(2, 0, 1, 3).reshape(16, -1)


@pytest.mark.parametrize("splits", [1, 2])
def test_adam_kernel_skips_dead_partials_and_dead_pack_slices(be, splits):
    """mnk_adam_multi, gt path: sentinel-filled dead slices + MNK_ADAM_UP1X1 give the p, m, v of zero-filled partials without the
    bit -- they are never loaded -- and, of packs pre-filled with a finite marker, the live slices come out bit-equal while the
    dead ones still hold the marker (without the bit every slice is written)"""
    live_f, live_d = _live(be, 0), _live(be, 1)
    g = torch.Generator().manual_seed(77)
    w = torch.randn(COUT, CIN, 1, 3, 3, generator=g) * 0.1
    m0, v0 = torch.randn(w.shape, generator=g) * 1e-3, torch.rand(w.shape, generator=g) * 1e-5
    parts = [_synthetic_partials(splits, c, live_f, 90 + c) for _, c in SOURCES]
    hyper = torch.tensor([2e-4, 0.5, 0.999, 1e-8, 0.0, 0.0, 1.0, 0.0, 1 - 0.5, 1 - 0.999], dtype=torch.float64).float()
    out = []
    for which, flag in ((0, 0), (1, 8)):
        P, M, V = be.t(w.clone()), be.t(m0.clone()), be.t(v0.clone())
        G = be.t(_sentinel(*w.shape))                                   # `g` is not read on the gt path
        wf = be.t(torch.full((be.query("mnk_conv3x3_up_packed_floats", COUT, C0, C1),), MARKER))
        w0 = be.t(torch.full((be.query("mnk_conv3x3_up_dgrad_packed_floats", COUT, C0),), MARKER))
        w1 = be.t(torch.full((be.query("mnk_conv3x3_up_dgrad_packed_floats", COUT, C1),), MARKER))
        gt = [be.t(p[which]) for p in parts]
        nb = be.query("mnk_adam_blocks", 0, COUT, C0, C1, 1)
        rows = [(P.data_ptr(), G.data_ptr(), M.data_ptr(), V.data_ptr(), w.numel(), wf.data_ptr(), w0.data_ptr(), w1.data_ptr(),
                 COUT, C0, C1, 0, 1 | 2 | 4 | flag, 0, gt[0].data_ptr(), gt[1].data_ptr(), splits, splits)]
        H = be.t(hyper.clone())
        be.call("mnk_adam_tick", H)
        be.call("mnk_adam_multi", _table(be, np.array(rows, dtype=ADAM_DESC)), 1, nb, H)
        be.sync()
        out.append((P.cpu(), M.cpu(), V.cpu()) + _pack_views(wf, w0, w1))
    base, got = out
    for a, b in zip(base[:3], got[:3]):
        assert bool(torch.isfinite(a).all()) and torch.equal(_bits(a), _bits(b))
    assert not torch.equal(base[0], w)
    for k, live in ((3, live_f), (4, live_d), (5, live_d)):
        for t in range(16):
            assert bool((base[k][t] != MARKER).all()), (k, t)           # the full emission wrote every slice
            if t in live:
                assert torch.equal(_bits(base[k][t]), _bits(got[k][t])), (k, t)
            else:
                assert bool((got[k][t] == MARKER).all()), (k, t)


@pytest.mark.parametrize("hs,ws", [(1, 1), (1, 2), (2, 1)])
def test_forward_and_data_gradient_need_exactly_the_live_pack_slices(be, hs, ws):
    """the live sets of the packs from the GEMMs themselves: a marker in EVERY slice the padding rule calls dead for this geometry
    changes no bit of y / dx, and a marker in any live slice does.  On the 1 x 1 source the rule's sets are the helper's; 1 x 2
    and 2 x 1 sources need eight slices of each pack, among them slices that are dead on 1 x 1"""
    x0, x1, dy = _inputs(hs, ws)
    g = torch.Generator().manual_seed(3)
    W = be.t(torch.randn(COUT, CIN, 1, 3, 3, generator=g) * 0.1)
    X0, X1, DY = be.t(to_nhwc(x0)), be.t(to_nhwc(x1)), be.t(to_nhwc(dy))
    wf = be.empty(be.query("mnk_conv3x3_up_packed_floats", COUT, C0, C1))
    w0 = be.empty(be.query("mnk_conv3x3_up_dgrad_packed_floats", COUT, C0))
    be.call("mnk_conv3x3_up_pack_fwd", W, wf, COUT, C0, C1)
    be.call("mnk_conv3x3_up_pack_dgrad", W, w0, COUT, CIN, 0, C0)
    chunks, dchunks = 3, 2
    nws = be.query("mnk_conv3x3_up_workspace_floats", N, hs, ws, C0, C1, COUT)
    nwd = be.query("mnk_conv3x3_up_dgrad_workspace_floats", N, hs, ws, COUT, C0)
    ldy = DY.shape[-1]

    # (one set of guarded buffers for all the launches of a form)
    Y, DX = be.empty(N, 2 * hs, 2 * ws, ldy), be.empty(N, hs, ws, X0.shape[-1])
    wsf, wsd = be.empty(max(nws, 1)), be.empty(max(nwd, 1))
    pf, pd = be.empty(wf.numel()), be.empty(w0.numel())

    def fwd(pack):
        pf.copy_(pack)
        Y.fill_(float("nan"))
        be.call("mnk_conv3x3_up_fwd", X0, X0.shape[-1], C0, X1, X1.shape[-1], C1, 0, pf, None, Y, ldy, N, hs, ws, COUT, wsf, nws, None)
        be.sync()
        return Y.cpu().clone()

    def dgrad(pack):
        pd.copy_(pack)
        DX.fill_(float("nan"))
        be.call("mnk_conv3x3_up_dgrad", DY, ldy, COUT, pd, DX, X0.shape[-1], N, hs, ws, C0, wsd, nwd)
        be.sync()
        return DX.cpu().clone()

    def marked(pack, view, taps, fwd_layout):
        p = pack.cpu().clone().view(view)
        for t in taps:
            if fwd_layout:
                p[t // 4, :, :, t % 4] = MARKER
            else:
                p[:, :, t] = MARKER
        return p.reshape(-1).to(be.device)

    for run, pack, view, dg in ((fwd, wf, (4, COUT, chunks, 4, 16), 0), (dgrad, w0, (C0, dchunks, 16, 16), 1)):
        if dg:
            live = [t for t in range(16) if _axis_live_dgrad(hs, t >> 2) and _axis_live_dgrad(ws, t & 3)]
        else:
            live = [t for t in range(16) if _axis_live(hs, (t >> 3) & 1, (t >> 1) & 1) and _axis_live(ws, (t >> 2) & 1, t & 1)]
        dead = [t for t in range(16) if t not in live]
        assert len(live) == 4 * hs * ws and (live == _live(be, dg) or hs * ws > 1)
        ref = run(pack)
        assert bool(torch.isfinite(ref).all())
        if dead:
            assert torch.equal(_bits(ref), _bits(run(marked(pack, view, dead, not dg)))), ("dead slices are in use", dg)
        for t in live:
            assert not torch.equal(_bits(ref), _bits(run(marked(pack, view, [t], not dg)))), ("a live slice is not in use", dg, t)


# ---- the registry: a weight whose last emission was partial and that then meets a larger source ------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("direct", [False, True], ids=["reduced", "tap-direct"])
def test_a_larger_source_after_a_partial_emission_gets_full_packs(be, direct, precision):
    """UpBlock3D: forward + backward + MnkAdam step on a 1 x 1 source (the step leaves the dead slices of the packs alone), then
    forwards on the 1 x 1 and on a 2 x 2 source -- the second needs every slice, so the entry is packed in full first and the bit
    stays off for this weight -- and another step: outputs and parameters bit-equal to the same sequence with up1x1_dead_taps = 0.
    precision: of the forwards and the step after the flagged step (the bf16 forms multiply the stale slices by zeros)."""
    from modules.util import UpBlock3D
    from mnk import ops as mops, optim as moptim
    g = torch.Generator().manual_seed(12)
    xa = torch.randn(4, 80, 1, 1, 1, generator=g)
    xb = torch.randn(4, 80, 1, 2, 2, generator=g)

    def run(knob):
        with tuning(be.lib, up1x1_dead_taps=knob):
            torch.manual_seed(8)
            blk = UpBlock3D(80, 24, kernel_size=(1, 3, 3), padding=(0, 1, 1)).to(be.device).train()
            opt = moptim.MnkAdam(blk.parameters(), lr=1e-3, betas=(0.5, 0.999))
            opt.tap_direct = direct
            XA, XB = be.t(xa), be.t(xb)
            outs, states = [], []

            def state():
                e = mops.pack_entry_of(blk.conv.weight)
                return (e.dead1x1, e.partial, e.full)

            def step(x):
                y = blk(x)
                outs.append(y.detach().cpu().clone())
                (y * y).mean().backward()
                opt.materialize_grads()
                ndirect = len(opt.reducer.direct)
                opt.step()
                opt.zero_grad()
                states.append(state() + (ndirect,))

            step(XA)
            with mops.training_precision(precision):
                step(XA)                           # the packs the flagged step left, on the geometry they were left for
                step(XB)                           # ... and on one that needs every slice
                step(XA)                           # the bit stays off: a full emission again
            be.sync()
            return outs, [p.detach().cpu().clone() for p in blk.parameters()], states

    (o0, p0, s0), (o1, p1, s1) = run(0), run(1)
    # (dead1x1, partial, full, layers the optimiser kernel read straight from the partials).  The last step of knob 1: the GEMM
    # of the 1 x 1 source still leaves its dead slices unwritten while the weight's packs are emitted in full -- the kernel's
    # one bit cannot say both, so the reduction (which has its own) sums those partials
    d = int(direct)
    assert s0 == [(False, False, False, d)] * 4, s0
    assert s1 == [(True, True, False, d), (True, True, False, d), (False, False, True, d), (False, False, True, 0)], s1
    for a, b in zip(o0 + p0, o1 + p1):
        assert bool(torch.isfinite(a).all()) and torch.equal(_bits(a), _bits(b))


# ---- the whole step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_moving_gif_training_steps_are_bit_equal_with_and_without_dead_taps():
    """moving-gif parameters at 64 x 64 (its three hourglasses reach 1 x 1 maps), batch 2, three TrainStep iterations: losses,
    generated tensors and every parameter bit-equal between up1x1_dead_taps = 0 and 1, eager and replayed; the replays (whose
    optimiser kernels read the deep levels' partials themselves) bit-equal to the eager iterations"""
    from oracle import cases
    from mnk import _lib, configs, engine
    from test_modules import build
    cfg = configs.get("moving-gif")
    dev = torch.device("cuda:0")
    src, drv = cases.synthetic_pair(2, 64, 64)
    x = {"source": src.to(dev), "video": drv.to(dev)}
    torch.manual_seed(0)
    mods = build(cfg)
    sds = []
    for i, m in enumerate(mods):
        sd = m.state_dict()
        cases.perturb_state_dict(sd, 7 + i)
        sds.append(sd)
    del mods

    def run(knob, use_graph):
        with tuning(_lib.lib(), up1x1_dead_taps=knob):
            mods = build(cfg)
            for m, sd in zip(mods, sds):
                m.load_state_dict(sd)
                m.to(dev)
            step = engine.TrainStep(*mods, cfg["train_params"], fused_adam=True, use_graph=use_graph)
            its = []
            for _ in range(3):
                g_l, d_l, gen = step.step(x)
                torch.cuda.synchronize()
                its.append([v.detach().reshape(-1).float().cpu().clone() for v in list(g_l) + list(d_l)] +
                           [gen[k].detach().cpu().clone() for k in sorted(gen) if torch.is_tensor(gen[k])] +
                           [p.detach().cpu().clone() for m in mods for p in m.parameters()])
            dead = sum(int(r["up1x1"]) for o in (step.opt_g, step.opt_k) for r in o.reducer.recs.values())
            return its, dead

    (e0, d0), (e1, d1), (g1, d2) = run(0, False), run(1, False), run(1, True)
    assert d0 == 0 and d1 >= 3 and d2 == d1, (d0, d1, d2)          # the three 1 x 1-source layers (per source) were taken
    for k in range(3):
        assert all(bool(torch.isfinite(t).all()) for t in e0[k])
        assert len(e0[k]) == len(e1[k]) == len(g1[k])
        for a, b, c in zip(e0[k], e1[k], g1[k]):
            assert torch.equal(_bits(a), _bits(b)), ("knob 0 / knob 1 differ in iteration", k)
            assert torch.equal(_bits(b), _bits(c)), ("replay / eager differ in iteration", k)
