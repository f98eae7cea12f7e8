"""The mnk_gru_* kernels (csrc/gru.hip) past one tile, one K chunk and one block: the smallest shapes at which a wave of a step
kernel takes a second K chunk, a second batch / hidden tile exists, the scalar form of the four-float loads runs, a GEMM has
tiles in M and N and several ragged K splits of a grouped operand, the column sums and the head have more than one block, and
every optional (NULL) argument is absent once.  Each result is compared with the float64 restatements of test_predictor.py;
the same quantity computed by stock float32 torch on the CPU sets the scale of the allowed error (`_close`), so no kernel is
measured against itself.  Outputs are NaN-filled guard-banded buffers with row pitches wider than their logical width: pad
columns must still be NaN afterwards, and the pad columns of the inputs are NaN too, so a read of one poisons the result.
Runs through the `be` fixture: on the CPU emulator and, with -m gpu, on the MI355X."""
import math

import pytest
import torch
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)
from test_predictor import _step_ref, _two_step_bwd_case, head64

NAN = float("nan")


def _w_scale(H):
    """the weight scale of test_predictor.perturbed: gate pre-activations of O(1) at any H"""
    return 0.3 * min(1.0, math.sqrt(64.0 / H))


def _close(name, got, stock, ref):
    """the rule of test_predictor._module_case: the native error may be 8 times the error of stock float32 torch (the same
    quantity, computed on the CPU) plus a floor of 2e-6 of the reference's magnitude"""
    got, stock, ref = got.detach().cpu().double(), stock.detach().double(), ref.detach()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    e_nat = float((got - ref).abs().max())
    e_stock = float((stock - ref).abs().max())
    floor = 2e-6 * max(1.0, float(ref.abs().max()))
    print("FIGURE %s: native %.3e stock %.3e floor %.3e" % (name, e_nat, e_stock, floor))
    assert e_nat <= 8 * e_stock + floor, (name, e_nat, e_stock, floor)


def _padded(be, x, ld, offset=0):
    """x [rows, w] on the backend inside a NaN-filled [rows, ld] buffer that starts `offset` floats into its allocation"""
    rows, w = x.shape
    flat = torch.full((offset + rows * ld,), NAN)
    flat[offset:].view(rows, ld)[:, :w] = x
    return be.t(flat)[offset:].view(rows, ld)


# ---- 1. forward step ---------------------------------------------------------------------------------------------------------
def _step_fwd(be, B, H, gemv_rows, ld_hp=None, hp_offset=0, with_gates=True):
    """one mnk_gru_step_fwd call at pitches ld_hp = H + 4, ld_gi = 3H + 2, ld_h = H + 8; returns (h [B, H], gates [B, 4H] | None)
    on the CPU and the (h, gates) of _step_ref in float64 and in float32"""
    g = torch.Generator().manual_seed(1000 * B + H)
    hp = torch.randn(B, H, generator=g)
    w_hh = torch.randn(3 * H, H, generator=g) * _w_scale(H)
    b_hh = torch.randn(3 * H, generator=g) * 0.2
    gi = torch.randn(B, 3 * H, generator=g)
    ld_hp = ld_hp or H + 4
    ld_gi, ld_h = 3 * H + 2, H + 8
    h = be.empty(B, ld_h)
    gates = be.empty(B, 4 * H) if with_gates else None
    be.lib.call("mnk_set_tuning", b"gru_gemv_rows", gemv_rows)
    try:
        be.call("mnk_gru_step_fwd", _padded(be, hp, ld_hp, hp_offset), ld_hp, be.t(w_hh), be.t(b_hh), _padded(be, gi, ld_gi), ld_gi,
                h, ld_h, gates, B, H)
        be.sync()
    finally:
        be.lib.call("mnk_set_tuning", b"gru_gemv_rows", 4)
    h = h.cpu()
    assert torch.isnan(h[:, H:]).all()
    ref = _step_ref(hp.double(), w_hh.double(), b_hh.double(), gi.double())
    stock = _step_ref(hp, w_hh, b_hh, gi)
    return h[:, :H], (gates.cpu() if with_gates else None), ref, stock


def _check_step_fwd(tag, H, h, gates, ref, stock):
    _close(tag + " h", h, stock[0], ref[0])
    for q, name in enumerate(("r", "z", "n", "hn")):
        _close(tag + " " + name, gates[:, q * H:(q + 1) * H], stock[1][:, q * H:(q + 1) * H], ref[1][:, q * H:(q + 1) * H])


@pytest.mark.parametrize("B,H", [(33, 132), (2, 131), (4, 260)])
def test_step_fwd_tile_form(be, B, H):
    """gru_step_fwd_kernel ("gru_gemv_rows" = 0).  (33, 132): blockIdx.y = 1 holds one batch row, blockIdx.x = 4 four hidden
    units, and H = 132 is five K chunks, so wave 0 takes chunks 0 and 4 (the second trip of `for c = w; c += 4`).  (2, 131):
    H % 4 != 0, every load is the scalar form of ld4 and the last chunk ends inside a group of four.  (4, 260): nine chunks
    (wave 0 takes three), the shape the GEMV form is checked at too"""
    h, gates, ref, stock = _step_fwd(be, B, H, 0)
    _check_step_fwd("tile B=%d H=%d" % (B, H), H, h, gates, ref, stock)


@pytest.mark.parametrize("how", ["ld_hp", "h_prev"])
def test_step_fwd_tile_form_scalar_loads_with_h_a_multiple_of_4(be, how):
    """vec == 0 at H % 4 == 0 (B = 3, H = 136): a row pitch ld_hp = H + 3 that is no multiple of four, or an h_prev that starts
    one float into its allocation (not 16-byte aligned); the fifth K chunk holds eight live k"""
    B, H = 3, 136
    h, gates, ref, stock = _step_fwd(be, B, H, 0, **({"ld_hp": H + 3} if how == "ld_hp" else {"hp_offset": 1}))
    _check_step_fwd("tile scalar " + how, H, h, gates, ref, stock)


@pytest.mark.parametrize("B,H,rows", [(8, 260, 8), (1, 261, 8), (4, 516, 4), (4, 260, 8)])
def test_step_fwd_gemv_form(be, B, H, rows):
    """gru_step_fwd_gemv_kernel.  (8, 260): B = GEMV_MAX_B, and k = 256 of `for k = 4 * lane; k += 256` is live for lane 0 alone.
    (1, 261): H % 4 != 0, scalar loads, lane 0's second trip ends after k = 260.  (4, 516): three trips, selected by the
    knob's default value 4.  (4, 260): the shape of the tile form's case (both meet the float64 reference; they need not be
    bitwise equal)"""
    h, gates, ref, stock = _step_fwd(be, B, H, rows)
    _check_step_fwd("gemv B=%d H=%d" % (B, H), H, h, gates, ref, stock)


@pytest.mark.parametrize("B,H,rows", [(33, 132, 0), (8, 260, 8)])
def test_step_fwd_without_gates(be, B, H, rows):
    """gates == NULL (the inference call) in the tile form and in the GEMV form: h meets the reference and equals the h of the
    call that saves the gates bit for bit"""
    h, _, ref, stock = _step_fwd(be, B, H, rows, with_gates=False)
    h_g, _, _, _ = _step_fwd(be, B, H, rows)
    _close("no gates B=%d H=%d h" % (B, H), h, stock[0], ref[0])
    assert torch.equal(h, h_g)


# ---- 2. backward step and gate backward ----------------------------------------------------------------------------------------
def _bwd_buffers(be, c, B, H):
    """the operands of the backward calls as the product lays them out, with wider pitches: dy [B, 2H + 1] = dy0 | dy1 | pad
    (mnk/gru.py passes dout[:, t] with ld_dy = T * H), h_{t-1} at ld_hp = H + 4, NaN pads"""
    f = lambda t: t.detach().float()
    dy = _padded(be, torch.cat([f(c.dy0), f(c.dy1)], 1), 2 * H + 1)
    return dy[:, :H], dy[:, H:], 2 * H + 1, _padded(be, f(c.h0), H + 4), _padded(be, f(c.h1), H + 4), H + 4


@pytest.mark.parametrize("B,H,dgh_offset", [(33, 132, 0), (2, 45, 0), (3, 40, 1)])
def test_step_bwd_wide_pitches(be, B, H, dgh_offset):
    """mnk_gru_gates_bwd, then mnk_gru_step_bwd with dh_out AND gates_prev (dh_out = dL/dh_1, and the gate gradients of step 0),
    then the dh0 form, against float64 autograd of two chained steps; ld_dy = 2H + 1, ld_hp = H + 4, ld_out = H + 5 with NaN pads.
    (33, 132): two batch tiles x five hidden tiles, 13 K chunks over four waves.  (2, 45): 3H = 135, vec == 0 and a last chunk of
    seven k.  (3, 40) with dgh one float into its allocation: vec == 0 at 3H % 4 == 0"""
    ref = _two_step_bwd_case(B, H, torch.float64, _w_scale(H))
    st = _two_step_bwd_case(B, H, torch.float32, _w_scale(H))
    f = lambda t: be.t(t.detach().float())
    dy0, dy1, ld_dy, h0, h1, ld_hp = _bwd_buffers(be, ref, B, H)
    w_hh, gates0, gates1 = f(ref.w_hh), f(ref.g0), f(ref.g1)
    dgi = [be.empty(B, 3 * H) for _ in range(2)]
    dgh_flat = [be.empty(dgh_offset + B * 3 * H) for _ in range(2)]
    dgh = [x[dgh_offset:].view(B, 3 * H) for x in dgh_flat]
    carry = be.empty(B, H)
    ld_out = H + 5
    dh1, dh0 = be.empty(B, ld_out), be.empty(B, ld_out)
    be.call("mnk_gru_gates_bwd", dy1, ld_dy, f(ref.dhn), gates1, h1, ld_hp, dgi[1], dgh[1], carry, B, H)
    be.call("mnk_gru_step_bwd", dgh[1], w_hh, carry, dy0, ld_dy, gates0, h0, ld_hp, dgi[0], dgh[0], dh1, ld_out, B, H)
    be.call("mnk_gru_step_bwd", dgh[0], w_hh, carry, None, 0, None, None, 0, None, None, dh0, ld_out, B, H)
    be.sync()
    for x in dgh_flat:
        assert torch.isnan(x[:dgh_offset]).all()
    for x in (dh1, dh0):
        assert torch.isnan(x[:, H:]).all()
    tag = "bwd B=%d H=%d " % (B, H)
    for name, got in (("dgi1", dgi[1]), ("dgh1", dgh[1]), ("dh1", dh1[:, :H]), ("dgi0", dgi[0]), ("dgh0", dgh[0]),
                      ("dh0", dh0[:, :H])):
        _close(tag + name, got, getattr(st, name), getattr(ref, name))


@pytest.mark.parametrize("term", ["dy", "dh_n"])
def test_gates_bwd_with_one_gradient_absent(be, term):
    """gru_gates_bwd_kernel with dh_n == NULL (dy alone, read at ld_dy = 2H + 1) and with dy == NULL (dh_n alone), B = 33, H = 132
    (17 blocks): the gate gradients and the carry dh * z of that term alone"""
    B, H = 33, 132
    ref = _two_step_bwd_case(B, H, torch.float64, _w_scale(H))
    st = _two_step_bwd_case(B, H, torch.float32, _w_scale(H))
    f = lambda t: be.t(t.detach().float())
    _, dy1, ld_dy, _, h1, ld_hp = _bwd_buffers(be, ref, B, H)
    dgi, dgh, carry = be.empty(B, 3 * H), be.empty(B, 3 * H), be.empty(B, H)
    if term == "dy":
        be.call("mnk_gru_gates_bwd", dy1, ld_dy, None, f(ref.g1), h1, ld_hp, dgi, dgh, carry, B, H)
        want, stock = ref.last(ref.dy1), st.last(st.dy1)
    else:
        be.call("mnk_gru_gates_bwd", None, 0, f(ref.dhn), f(ref.g1), h1, ld_hp, dgi, dgh, carry, B, H)
        want, stock = ref.last(ref.dhn), st.last(st.dhn)
    be.sync()
    for name, got, s, r in zip(("dgi", "dgh", "carry"), (dgi, dgh, carry), stock, want):
        _close("gates_bwd %s alone: %s" % (term, name), got, s, r)


# ---- 3. GEMM -----------------------------------------------------------------------------------------------------------------
def _gemm(be, M, N, K, A, B, bias, C, ldc):
    """C = A B^T (+ bias) on plain row-major operands A [M, K], B [N, K]"""
    ws_n = be.query("mnk_gru_gemm_workspace_floats", M, N, K)
    be.call("mnk_gru_gemm", 0, 1, M, N, K, A, K, 0, 0, B, K, 0, 0, bias, C, ldc, be.empty(max(ws_n, 1)), ws_n)
    be.sync()
    return ws_n


@pytest.mark.parametrize("K", [23, 1100])
def test_gemm_without_bias(be, K):
    """bias == NULL in the GEMM kernel's epilogue (K = 23) and in the split-K reduce (K = 1100): the product alone"""
    M, N = 40, 24
    torch.manual_seed(K)
    A, B = torch.randn(M, K), torch.randn(N, K)
    C = be.empty(M, N + 3)
    ws_n = _gemm(be, M, N, K, be.t(A), be.t(B), None, C, N + 3)
    assert (ws_n > 0) == (K == 1100)
    C = C.cpu()
    assert torch.isnan(C[:, N:]).all()
    ref, scale = A.double() @ B.double().t(), A.double().abs() @ B.double().abs().t()
    assert ((C[:, :N].double() - ref).abs() <= 2e-7 * scale + 1e-6).all()


def test_gemm_k_zero_is_the_bias(be):
    """K == 0: the empty sum, every row of C is the bias (350 elements: two blocks of the reduce kernel that writes it) and the
    pad columns stay untouched; A and B are not read (NULL)"""
    M, N = 5, 70
    bias = torch.randn(N, generator=torch.Generator().manual_seed(0))
    C = be.empty(M, N + 3)
    assert be.query("mnk_gru_gemm_workspace_floats", M, N, 0) == 0
    be.call("mnk_gru_gemm", 0, 1, M, N, 0, None, 0, 0, 0, None, 0, 0, 0, be.t(bias), C, N + 3, None, 0)
    be.sync()
    C = C.cpu()
    assert torch.isnan(C[:, N:]).all()
    assert torch.equal(C[:, :N], bias.expand(M, N))


@pytest.mark.parametrize("M,N", [(0, 24), (40, 0)])
def test_gemm_with_no_rows_or_columns_writes_nothing(be, M, N):
    """M == 0 or N == 0: success, and a NaN-filled C is still all NaN"""
    K = 23
    A, B, bias = be.t(torch.randn(40, K)), be.t(torch.randn(24, K)), be.t(torch.randn(24))
    C = be.empty(40, 27)
    _gemm(be, M, N, K, A, B, bias, C, 27)
    assert torch.isnan(C.cpu()).all()


def test_gemm_split_k_is_deterministic(be):
    """the three-split case (70, 130, 1540) twice: the partial planes are summed in a fixed order, so the results are bitwise
    equal"""
    M, N, K = 70, 130, 1540
    torch.manual_seed(7)
    A, B, bias = be.t(torch.randn(M, K)), be.t(torch.randn(N, K)), be.t(torch.randn(N))
    out = []
    for _ in range(2):
        C = be.empty(M, N)
        assert _gemm(be, M, N, K, A, B, bias, C, N) == 3 * M * N
        out.append(C.cpu())
    assert not torch.isnan(out[0]).any()
    assert torch.equal(out[0], out[1])


# ---- 4. column sums ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(0, 300), (1, 300), (129, 300), (8193, 300), (129, 520)])
def test_colsum_past_one_column_block(be, rows, cols):
    """cols = 300 (blockIdx.x = 1 holds 44 columns) at ld = 307 with NaN pad columns; rows = 0 (x == NULL: 300 exact zeros), 1,
    129 (two row blocks: 65 + 64 rows) and 8193 (64 row blocks of rpb = 129 > 128 rows, the last with 66).  cols = 520: a third
    column block, the fewest at which a column stride of 128 in place of 256 leaves columns unwritten (at 300 the blocks of such a
    stride overlap and still cover every column).  Each output is a sequential fp32 sum of at most rpb terms followed by one of
    nb terms: |got - ref| <= (rpb + nb) 2^-24 sum|x| per column"""
    ld = cols + 7
    x = torch.randn(rows, ld, generator=torch.Generator().manual_seed(rows))
    x[:, cols:] = NAN
    ws_n = be.query("mnk_gru_colsum_workspace_floats", rows, cols)
    assert ws_n > 0 and ws_n % cols == 0
    nb = ws_n // cols
    rpb = -(-rows // nb)
    assert nb == {0: 1, 1: 1, 129: 2, 8193: 64}[rows] and (rows != 8193 or rpb > 128)
    out = be.empty(cols + 4)
    be.call("mnk_gru_colsum", be.t(x) if rows else None, ld, rows, cols, out, be.empty(ws_n), ws_n)
    be.sync()
    out = out.cpu()
    assert torch.isnan(out[cols:]).all()
    if rows == 0:
        assert torch.equal(out[:cols], torch.zeros(cols))
        return
    xd = x[:, :cols].double()
    bound = (rpb + nb) * 2.0 ** -24 * xd.abs().sum(0)
    err = (out[:cols].double() - xd.sum(0)).abs()
    print("FIGURE colsum rows=%d: max error / bound %.3e" % (rows, float((err / bound).max())))
    assert (err <= bound).all()


# ---- 5. head -----------------------------------------------------------------------------------------------------------------
def _head_case(has_var, F, rows=67, K=10):
    """y [rows, K * F] (670 key points: three blocks, the last with 158) and, per dtype, the head's outputs and the gradient of
    <mean, gm> (+ <var, gv>) and of each term alone"""
    g = torch.Generator().manual_seed(10 + F)
    y = torch.randn(rows, K * F, generator=g)
    gm, gv = torch.randn(rows, K, 2, generator=g), torch.randn(rows, K, 2, 2, generator=g)

    def run(dtype):
        yd = y.to(dtype).requires_grad_()
        out = head64(yd.view(1, rows, -1), K, has_var)
        mean = out["mean"].reshape(rows, K, 2)
        terms = {"mean": (mean * gm.to(dtype)).sum()}
        res = {"mean": mean.detach()}
        if has_var:
            var = out["var"].reshape(rows, K, 2, 2)
            terms["var"] = (var * gv.to(dtype)).sum()
            res["var"] = var.detach()
        for k, L in terms.items():
            res["dy " + k] = torch.autograd.grad(L, yd, retain_graph=True)[0]
        res["dy"] = sum(res["dy " + k] for k in terms)
        return res
    return y, gm, gv, run(torch.float64), run(torch.float32)


@pytest.mark.parametrize("has_var,F", [(True, 8), (False, 3)])
def test_head_three_blocks_and_spare_features(be, has_var, F):
    """gru_head_fwd/bwd_kernel at rows * num_kp = 670 (blockIdx.x = 0..2, the last block ragged) with more features per key point
    than the head reads (8 > 6 with has_var, 3 > 2 without): the spare features get exactly 0 in dy"""
    rows, K = 67, 10
    y, gm, gv, ref, st = _head_case(has_var, F)
    mean, var = be.empty(rows, K, 2), be.empty(rows, K, 2, 2) if has_var else None
    dy = be.empty(rows, K * F)
    be.call("mnk_gru_head_fwd", be.t(y), rows, K, F, int(has_var), mean, var)
    be.call("mnk_gru_head_bwd", be.t(y), be.t(gm), be.t(gv) if has_var else None, rows, K, F, int(has_var), dy)
    be.sync()
    _close("head mean", mean, st["mean"], ref["mean"])
    if has_var:
        _close("head var", var, st["var"], ref["var"])
    _close("head dy", dy, st["dy"], ref["dy"])
    assert (dy.cpu().view(rows, K, F)[..., 6 if has_var else 2:] == 0).all()


@pytest.mark.parametrize("given", ["var", "mean"])
def test_head_bwd_with_one_gradient_absent(be, given):
    """gru_head_bwd_kernel with dmean == NULL (dvar given) and with dvar == NULL (dmean given), has_var = 1, 8 features: the
    autograd gradient of that output alone"""
    rows, K, F = 67, 10, 8
    y, gm, gv, ref, st = _head_case(True, F)
    dy = be.empty(rows, K * F)
    be.call("mnk_gru_head_bwd", be.t(y), be.t(gm) if given == "mean" else None, be.t(gv) if given == "var" else None, rows, K, F, 1,
            dy)
    be.sync()
    _close("head dy of %s alone" % given, dy, st["dy " + given], ref["dy " + given])
    assert (dy.cpu().view(rows, K, F)[..., 6:] == 0).all()
