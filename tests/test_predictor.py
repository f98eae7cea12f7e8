"""The key-point GRU of the prediction task (mnk.predictor.PredictionModule on csrc/gru.hip): every mnk_gru_* kernel against a
float64 restatement, the module's forward and every gradient against float64 autograd, the construction contract of the
reference's modules/prediction_module.py, stacked layers, determinism, and the MNK_NATIVE_PREDICTION switch.  Kernel and module
tests run through the `be` fixture: on the CPU emulator and, with -m gpu, on the MI355X."""
import os
import subprocess
import sys

import pytest
import torch
from torch import nn
from _guard import be  # noqa: F401  (guard-banded buffers, checked calls)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MNK_REFERENCE_ROOT", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "modules", "prediction_module.py")),
                                     reason="needs a checkout of the reference (MNK_REFERENCE_ROOT)")


# ---- float64 restatements of nn.GRU (batch_first) / nn.Linear / prediction_module.py:33-42 ----------------------------------
def gru64(x, h0, w_ih, w_hh, b_ih, b_hh):
    B, T, _ = x.shape
    H = w_hh.shape[1]
    h = h0 if h0 is not None else x.new_zeros(B, H)
    outs = []
    for t in range(T):
        gi = x[:, t] @ w_ih.t() + b_ih
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        outs.append(h)
    return torch.stack(outs, 1), h


def head64(y, num_kp, has_var):
    bs, d, _ = y.shape
    o = y.view(bs, d, num_kp, -1)
    res = {"mean": torch.tanh(o[..., :2])}
    if has_var:
        v = o[..., 2:6].reshape(bs, d, num_kp, 2, 2)
        res["var"] = v.transpose(-1, -2) @ v
    return res


def predictor64(params, kp, num_layers, h0=None):
    """params: name -> float64 leaf; the reference's forward (prediction_module.py:28-44) with gru64 / a float64 linear."""
    bs, d, num_kp, _ = kp["mean"].shape
    x = torch.cat([kp[k].reshape(bs, d, -1) for k in ("mean", "var") if k in kp], -1)
    hn = []
    for l in range(num_layers):
        x, h = gru64(x, None if h0 is None else h0[l], *(params["rnn.%s_l%d" % (n, l)]
                                                         for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
        hn.append(h)
    y = x @ params["linear.weight"].t() + params["linear.bias"]
    return head64(y, num_kp, "var" in kp), torch.stack(hn, 0)


def make_kp(B, T, num_kp, matrix, seed, device="cpu"):
    """key-point batch as prediction.py feeds it, the tensors given as NON-contiguous slices of larger ones"""
    g = torch.Generator().manual_seed(seed)
    kp = {"mean": (torch.rand(B, T, num_kp, 3, generator=g) * 2 - 1)[..., :2]}
    if matrix:
        v = torch.randn(B, T, num_kp, 2, 2, generator=g) * 0.3
        kp["var"] = (v.transpose(-1, -2) @ v + 0.05 * torch.eye(2)).transpose(0, 1).contiguous().transpose(0, 1)
    return {k: v.to(device) for k, v in kp.items()}


def perturbed(mod, seed):
    """larger weights than nn.GRU's init (its U(-1/sqrt(H), 1/sqrt(H)) keeps every gate near 1/2); pre-activations of O(1) at any H"""
    g = torch.Generator().manual_seed(seed)
    sd = mod.state_dict()
    f = min(1.0, (64.0 / mod.rnn.hidden_size) ** 0.5)
    for k in sd:
        sd[k] = sd[k] + torch.randn(sd[k].shape, generator=g) * (0.3 * f if "weight" in k else 0.2)
    mod.load_state_dict(sd)
    return mod


def _loss(out, seed):
    g = torch.Generator().manual_seed(seed)
    s = 0
    for k in sorted(out):
        w = torch.randn(out[k].shape, generator=g, dtype=torch.float64).to(out[k].device)
        s = s + (out[k].double() * w).sum()
    return s


# ---- kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transA,transB", [(0, 1), (0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K,grouped", [
    (37, 45, 23, False), (70, 24, 60, True), (40, 24, 1100, False),
    (70, 130, 23, False),       # 2 x 3 tiles (blockIdx.y = 1 with n0 = 64, 128), ragged in M and N, K not a multiple of 16
    (5, 200, 3, False),         # K < 16: one partly filled K step; four N tiles
    (70, 130, 1540, True),      # three K splits (chunks 528, 528, 484: the last ends inside a 16-wide step) of a grouped K-major
])                              # operand, on 2 x 3 tiles: the shape of the dW_ih GEMM (K = T * B)
def test_gemm_against_fp64(be, transA, transB, M, N, K, grouped):
    """all four operand orientations, grouped rows (a [G, R, C] view read in (r, g) order), split-K (K = 1100 on one tile, K = 1540
    on six), more than one tile in M and N, bias, an output row pitch wider than N whose pad columns stay untouched"""
    torch.manual_seed(M + N + K + 2 * transA + transB)
    A = torch.randn(K, M) if transA else torch.randn(M, K)
    B = torch.randn(N, K) if transB else torch.randn(K, N)
    bias = torch.randn(N)

    def operand(X):
        if not grouped or X.shape[0] % 5:
            return be.t(X), X.shape[1], 0, 0
        # rows r = g * R + i stored at g * C + i * (G * C): a [G, R, C] view of a [R, G, C] tensor
        R, C = X.shape[0] // 5, X.shape[1]
        store = be.t(X.view(5, R, C).transpose(0, 1).contiguous())          # [R, 5, C]
        return store, 5 * C, R, C

    a, lda, ag, ldag = operand(A)
    b, ldb, bg, ldbg = operand(B)
    ldc = N + 3
    C = be.empty(M, ldc)
    ws_n = be.query("mnk_gru_gemm_workspace_floats", M, N, K)
    if K == 1100:
        assert ws_n > 0
    if K == 1540:
        assert ws_n == 3 * M * N
    ws = be.empty(max(ws_n, 1))
    be.call("mnk_gru_gemm", transA, transB, M, N, K, a, lda, ag, ldag, b, ldb, bg, ldbg, be.t(bias), C, ldc, ws, ws_n)
    be.sync()
    ref = (A.double().t() if transA else A.double()) @ (B.double().t() if transB else B.double()) + bias.double()
    scale = ((A.double().abs().t() if transA else A.double().abs()) @ (B.double().abs().t() if transB else B.double().abs()))
    C = C.cpu()
    assert torch.isnan(C[:, N:]).all()
    assert ((C[:, :N].double() - ref).abs() <= 2e-7 * scale + 1e-6).all()


def test_colsum_against_fp64(be):
    torch.manual_seed(3)
    x = torch.randn(300, 77)
    ws_n = be.query("mnk_gru_colsum_workspace_floats", 300, 70)
    out = be.empty(72)
    be.call("mnk_gru_colsum", be.t(x), 77, 300, 70, out, be.empty(ws_n), ws_n)
    be.sync()
    out = out.cpu()
    assert torch.isnan(out[70:]).all()
    assert torch.allclose(out[:70].double(), x[:, :70].double().sum(0), atol=1e-5)


def _step_ref(hp, w_hh, b_hh, gi):
    H = w_hh.shape[1]
    gh = hp @ w_hh.t() + b_hh
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    hn = gh[:, 2 * H:]
    n = torch.tanh(gi[:, 2 * H:] + r * hn)
    return (1 - z) * n + z * hp, torch.cat([r, z, n, hn], 1)


@pytest.mark.parametrize("gemv", [0, 8])
@pytest.mark.parametrize("B,H", [(1, 40), (3, 72), (5, 40)])
def test_step_fwd_against_fp64(be, B, H, gemv):
    """one time step, both forms (the GEMV form up to "gru_gemv_rows" batch rows, the MFMA tile form above), row pitches wider
    than H / 3H with untouched pads"""
    torch.manual_seed(B * H + gemv)
    hp = torch.randn(B, H + 4)
    w_hh, b_hh = torch.randn(3 * H, H) * 0.3, torch.randn(3 * H) * 0.2
    gi = torch.randn(B, 3 * H + 2)
    h = be.empty(B, H + 8)
    gates = be.empty(B, 4 * H)
    be.lib.call("mnk_set_tuning", b"gru_gemv_rows", gemv)
    try:
        be.call("mnk_gru_step_fwd", be.t(hp), H + 4, be.t(w_hh), be.t(b_hh), be.t(gi), 3 * H + 2, h, H + 8, gates, B, H)
        be.sync()
    finally:
        be.lib.call("mnk_set_tuning", b"gru_gemv_rows", 4)
    href, gref = _step_ref(hp[:, :H].double(), w_hh.double(), b_hh.double(), gi[:, :3 * H].double())
    h, gates = h.cpu(), gates.cpu()
    assert torch.isnan(h[:, H:]).all()
    assert (h[:, :H].double() - href).abs().max() < 2e-6
    assert (gates.double() - gref).abs().max() < 2e-5 * max(1.0, float(gref.abs().max()))


def _two_step_bwd_case(B, H, dtype=torch.float64, w_scale=0.3):
    """Two chained GRU steps h0 -> h1 -> h2 with L = <h1, dy0> + <h2, dy1 + dhn>, computed with autograd in `dtype` (the inputs
    are drawn in float32, so every dtype sees the same values).  Returns a namespace of the inputs (w_hh, b_hh, h0, gi0, gi1,
    dy0, dy1, dhn), the forward values the kernels are handed (h1, the saved gates g0, g1 = r | z | n | hn) and the gradients:
    dgi_t = dL/d(gi_t), dgh_t = dL/d(h_{t-1} W_hh^T + b_hh), dh1 = dL/dh_1 (dy0 included), dh0 = dL/dh_0, and last(dh): the
    last step's (dgi1, dgh1, carry) for dL/dh_2 = dh alone (one term of dy1 + dhn)."""
    from types import SimpleNamespace
    torch.manual_seed(B + H)
    w_hh = (torch.randn(3 * H, H) * w_scale).to(dtype)
    b_hh = (torch.randn(3 * H) * 0.2).to(dtype)
    h0 = torch.randn(B, H).to(dtype).requires_grad_()
    gi0, gi1 = torch.randn(B, 3 * H).to(dtype), torch.randn(B, 3 * H).to(dtype)
    h1, g0 = _step_ref(h0, w_hh, b_hh, gi0)
    h1.retain_grad()
    h2, g1 = _step_ref(h1, w_hh, b_hh, gi1)
    dy1, dy0 = torch.randn(B, H).to(dtype), torch.randn(B, H).to(dtype)
    dhn = torch.randn(B, H).to(dtype)
    # gradients of the pre-activations: dGi_t = d(gi_t), dGh_t = d(h_{t-1} W_hh^T + b_hh)
    gi0.requires_grad_(), gi1.requires_grad_()
    gh0 = (h0 @ w_hh.t() + b_hh).detach().requires_grad_()
    gh1 = (h1 @ w_hh.t() + b_hh).detach().requires_grad_()

    def cell(hp, gi, gh):
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        return (1 - z) * n + z * hp
    h1c = cell(h0.detach(), gi0, gh0).detach().requires_grad_()
    h2c = cell(h1c, gi1, gh1)
    L = (h2c * (dy1 + dhn)).sum()
    L.backward()
    dh1 = h1c.grad + gh1.grad @ w_hh + dy0       # dL/dh_1, the output's gradient at t = 0 included
    (cell(h0, gi0, gh0) * dh1).sum().backward()

    def last(dh):
        a, b = gi1.detach().requires_grad_(), gh1.detach().requires_grad_()
        da, db = torch.autograd.grad((cell(h1c.detach(), a, b) * dh).sum(), (a, b))
        return da, db, dh * g1.detach()[:, H:2 * H]
    return SimpleNamespace(w_hh=w_hh, b_hh=b_hh, h0=h0, h1=h1, gi0=gi0, gi1=gi1, g0=g0, g1=g1, dy0=dy0, dy1=dy1, dhn=dhn,
                           dgi1=gi1.grad, dgh1=gh1.grad, dgi0=gi0.grad, dgh0=gh0.grad, dh1=dh1.detach(),
                           dh0=gh0.grad @ w_hh + h0.grad, last=last)


@pytest.mark.parametrize("B,H", [(1, 40), (5, 72), (33, 40)])
def test_step_bwd_against_fp64(be, B, H):
    """gates backward of the last step, then one fused step backward (dh_{t-1} + the gate backward of step t - 1) and the final
    dh0 form, against float64 autograd of two GRU steps"""
    c = _two_step_bwd_case(B, H)
    w_hh, h0, h1, g0, g1, dy0, dy1, dhn = c.w_hh, c.h0, c.h1, c.g0, c.g1, c.dy0, c.dy1, c.dhn
    dgi1_ref, dgh1_ref, dgi0_ref, dgh0_ref, dh0_ref = c.dgi1, c.dgh1, c.dgi0, c.dgh0, c.dh0

    f = lambda t: be.t(t.detach().float())
    gates0, gates1 = f(g0), f(g1)
    dgi, dgh = be.empty(2, B, 3 * H), be.empty(2, B, 3 * H)
    carry, dh0 = be.empty(B, H), be.empty(B, H)
    be.call("mnk_gru_gates_bwd", f(dy1), H, f(dhn), gates1, f(h1), H, dgi[1], dgh[1], carry, B, H)
    be.call("mnk_gru_step_bwd", dgh[1], f(w_hh), carry, f(dy0), H, gates0, f(h0), H, dgi[0], dgh[0], None, H, B, H)
    be.call("mnk_gru_step_bwd", dgh[0], f(w_hh), carry, None, 0, None, None, 0, None, None, dh0, H, B, H)
    be.sync()
    for got, ref in ((dgi[1], dgi1_ref), (dgh[1], dgh1_ref), (dgi[0], dgi0_ref), (dgh[0], dgh0_ref), (dh0, dh0_ref)):
        assert (got.cpu().double() - ref).abs().max() < 1e-5 * max(1.0, float(ref.abs().max())), (got, ref)


@pytest.mark.parametrize("has_var", [True, False])
def test_head_fwd_bwd_against_fp64(be, has_var):
    torch.manual_seed(int(has_var))
    rows, K = 7, 4
    F = 6 if has_var else 2
    y = torch.randn(rows, K * F).double().requires_grad_()
    out = head64(y.view(1, rows, -1), K, has_var)
    mean, var = be.empty(rows, K, 2), be.empty(rows, K, 2, 2) if has_var else None
    be.call("mnk_gru_head_fwd", be.t(y.detach().float()), rows, K, F, int(has_var), mean, var)
    gm = torch.randn(rows, K, 2).double()
    gv = torch.randn(rows, K, 2, 2).double()
    L = (out["mean"].view(rows, K, 2) * gm).sum() + ((out["var"].view(rows, K, 2, 2) * gv).sum() if has_var else 0)
    L.backward()
    dy = be.empty(rows, K * F)
    be.call("mnk_gru_head_bwd", be.t(y.detach().float()), be.t(gm.float()), be.t(gv.float()) if has_var else None, rows, K, F,
            int(has_var), dy)
    be.sync()
    assert (mean.cpu().double() - out["mean"].view(rows, K, 2)).abs().max() < 1e-6
    if has_var:
        assert (var.cpu().double() - out["var"].view(rows, K, 2, 2)).abs().max() < 1e-5
    assert (dy.cpu().double() - y.grad).abs().max() < 1e-5


# ---- the module -------------------------------------------------------------------------------------------------------------
def _build(num_kp, matrix, H, num_layers=1, dropout=0.0, seed=0):
    from mnk.predictor import PredictionModule
    torch.manual_seed(seed)
    return perturbed(PredictionModule(num_kp=num_kp, kp_variance="matrix" if matrix else 0.01, num_features=H,
                                      num_layers=num_layers, dropout=dropout), seed + 100)


def _module_case(be, B, T, num_kp, matrix, H, num_layers=1, with_h0=False, seed=0):
    """forward + every gradient of the native module vs float64 autograd; the native error may be a small factor of the float32
    stock nn.GRU's own error (plus a floor)"""
    mod = _build(num_kp, matrix, H, num_layers, seed=seed)

    def refuse(*a, **k):
        raise AssertionError("the parameter holder nn.GRU was called")
    mod.rnn.forward = refuse
    params64 = {k: v.detach().double().requires_grad_() for k, v in mod.named_parameters()}
    kp = make_kp(B, T, num_kp, matrix, seed + 1)
    h0 = torch.randn(num_layers, B, H) * 0.5 if with_h0 else None

    # float64 reference and the float32 stock module (the reference's own computation) on the CPU
    kp64 = {k: v.double().requires_grad_() for k, v in kp.items()}
    h064 = h0.double().requires_grad_() if with_h0 else None
    out64, hn64 = predictor64(params64, kp64, num_layers, h064)
    (_loss(out64, seed + 2) + (hn64 * 0.5).sum()).backward()

    stock = nn.ModuleDict({"rnn": nn.GRU(mod.rnn.input_size, H, num_layers, batch_first=True),
                           "linear": nn.Linear(H, mod.linear.out_features)})
    stock.load_state_dict(mod.state_dict())
    kps = {k: v.clone().requires_grad_() for k, v in kp.items()}
    h0s = h0.clone().requires_grad_() if with_h0 else None
    xs = torch.cat([kps[k].reshape(B, T, -1) for k in ("mean", "var") if k in kps], -1)
    os_, hns = stock["rnn"](xs, h0s)
    outs = head64(stock["linear"](os_), num_kp, matrix)
    (_loss(outs, seed + 2) + (hns * 0.5).sum()).backward()

    # native, through net() (h0, h_n) and the module's head
    mod.to(be.device)
    kpn = {k: v.to(be.device).requires_grad_() for k, v in kp.items()}
    h0n = h0.to(be.device).requires_grad_() if with_h0 else None
    xn = torch.cat([kpn[k].reshape(B, T, -1) for k in ("mean", "var") if k in kpn], -1)
    y, hnn = mod.net(xn, h0n)
    from mnk.gru import HeadFn
    o = HeadFn.apply(y, num_kp, matrix)
    outn = {"mean": o[0], "var": o[1]} if matrix else {"mean": o}
    (_loss(outn, seed + 2) + (hnn.double() * 0.5).sum()).backward()
    be.sync()

    pairs = [("out " + k, outn[k], outs[k], out64[k]) for k in out64] + [("h_n", hnn, hns, hn64)]
    pairs += [("grad " + k, dict(mod.named_parameters())[k].grad, dict(stock.named_parameters())[k].grad, params64[k].grad)
              for k in params64]
    pairs += [("grad kp " + k, kpn[k].grad, kps[k].grad, kp64[k].grad) for k in kp]
    if with_h0:
        pairs.append(("grad h0", h0n.grad, h0s.grad, h064.grad))
    for name, got, st, ref in pairs:
        assert got is not None, name
        e_nat = float((got.detach().cpu().double() - ref.detach()).abs().max())
        e_stock = float((st.detach().double() - ref.detach()).abs().max())
        floor = 2e-6 * max(1.0, float(ref.detach().abs().max()))
        assert e_nat <= 8 * e_stock + floor, (name, e_nat, e_stock, floor)
    return mod, kp


@pytest.mark.parametrize("B,T,num_kp,matrix,H,with_h0", [
    (1, 5, 10, True, 40, False),        # I = 60, 'matrix' variance, batch 1 (GEMV form of the step)
    (3, 1, 10, False, 72, True),        # I = 20, float kp_variance (no 'var' key), one step, h0 given
    (5, 5, 4, True, 72, True),          # I = 24 (shapes.yaml), the MFMA tile form of the step
    (5, 5, 10, False, 40, False),
    (33, 3, 4, True, 132, True),        # two batch tiles, five hidden tiles / K chunks; N = cols = 396 in the GEMMs / column sums
])
def test_module_forward_and_gradients_against_fp64(be, B, T, num_kp, matrix, H, with_h0):
    _module_case(be, B, T, num_kp, matrix, H, with_h0=with_h0, seed=B * 7 + T)


def test_two_layers_run_natively(be):
    """num_layers = 2 with dropout 0 stacks the native layers (the module's nn.GRU is never called)"""
    _module_case(be, 3, 4, 4, True, 40, num_layers=2, with_h0=True, seed=11)


def test_dropout_between_layers_in_training_is_the_stock_path():
    """dropout > 0 with stacked layers in training mode: nn.GRU's own dropout masks (RNG parity), i.e. the reference's computation
    exactly; in evaluation mode the same module runs natively"""
    from mnk.predictor import PredictionModule
    torch.manual_seed(5)
    mod = PredictionModule(num_kp=4, kp_variance="matrix", num_features=24, num_layers=2, dropout=0.5)
    stock = _StockPredictor(num_kp=4, kp_variance="matrix", num_features=24, num_layers=2, dropout=0.5)
    stock.load_state_dict(mod.state_dict())
    kp = make_kp(2, 3, 4, True, 9)
    torch.manual_seed(123)
    a = mod(kp)
    torch.manual_seed(123)
    b = stock(kp)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    (sum(v.sum() for v in a.values())).backward()
    (sum(v.sum() for v in b.values())).backward()
    for (n, p), q in zip(mod.named_parameters(), stock.parameters()):
        assert torch.equal(p.grad, q.grad), n


class _StockPredictor(nn.Module):
    """modules/prediction_module.py restated on stock torch (the fall-back the native module must equal bit for bit)"""

    def __init__(self, num_kp, kp_variance, num_features, num_layers, dropout):
        super().__init__()
        input_size = num_kp * (2 + 4 * (kp_variance == 'matrix'))
        self.rnn = nn.GRU(input_size=input_size, hidden_size=num_features, num_layers=num_layers, dropout=dropout, batch_first=True)
        self.linear = nn.Linear(num_features, input_size)

    def forward(self, kp_batch):
        bs, d, num_kp, _ = kp_batch['mean'].shape
        inputs = [kp_batch['mean'].contiguous().view(bs, d, -1)]
        if 'var' in kp_batch:
            inputs.append(kp_batch['var'].contiguous().view(bs, d, -1))
        output, _ = self.rnn(torch.cat(inputs, dim=-1))
        init_shape = output.shape
        output = self.linear(output.contiguous().view(-1, output.shape[-1])).view(init_shape[0], init_shape[1], -1)
        output = output.view(bs, d, num_kp, -1)
        res = {'mean': torch.tanh(output[:, :, :, :2])}
        if 'var' in kp_batch:
            var = output[:, :, :, 2:].reshape(bs, d, num_kp, 2, 2)
            res['var'] = torch.matmul(var.permute(0, 1, 2, 4, 3), var)
        return res


def test_construction_contract():
    """same seed -> the same parameters and state_dict keys as nn.GRU followed by nn.Linear (the reference's RNG order)"""
    from mnk.predictor import PredictionModule
    for kw in ({}, {"num_kp": 4, "kp_variance": "matrix", "num_features": 24, "num_layers": 2, "dropout": 0.0}):
        torch.manual_seed(42)
        mod = PredictionModule(**kw)
        a = dict(num_kp=10, kp_variance=0.01, num_features=1024, num_layers=1, dropout=0.5)
        a.update(kw)
        torch.manual_seed(42)
        stock = _StockPredictor(**a)
        sa, sb = mod.state_dict(), stock.state_dict()
        assert list(sa) == list(sb)
        assert list(sa)[:4] == ["rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0"]
        assert list(sa)[-2:] == ["linear.weight", "linear.bias"]
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k


def test_forward_matches_stock_and_is_deterministic(be):
    """forward() on a key-point batch equals the stock module within the fp32 rule, and two forward + backward runs are bitwise
    equal (no atomics; split-K partials summed in a fixed order)"""
    mod = _build(4, True, 40, seed=3).to(be.device)
    kp = make_kp(5, 4, 4, True, 4, be.device)
    runs = []
    for _ in range(2):
        mod.zero_grad(set_to_none=True)
        kpr = {k: v.clone().requires_grad_() for k, v in kp.items()}
        out = mod(kpr)
        _loss(out, 1).backward()
        be.sync()
        runs.append([out["mean"].detach().cpu(), out["var"].detach().cpu()] + [p.grad.cpu() for p in mod.parameters()]
                    + [kpr[k].grad.cpu() for k in sorted(kpr)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_cpu_tensors_raise_on_a_device_build():
    from mnk import _lib
    from mnk.predictor import PredictionModule
    if not os.path.exists(_lib.DEFAULT_LIB):
        pytest.skip("the gfx950 library is not built")
    lib = _lib.lib()
    if not lib.is_device_build:
        pytest.skip("the emulator library is bound")
    mod = PredictionModule(num_kp=2, kp_variance=0.01, num_features=8, dropout=0.0)
    with pytest.raises(_lib.MnkError):
        mod(make_kp(1, 2, 2, False, 0))


@needs_reference
def test_equals_the_reference_class(be):
    """the reference's modules/prediction_module.py, imported from its tree: the same parameters for the same seed; outputs and
    gradients on shared weights within the fp32 rule"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_prediction_module", os.path.join(REF, "modules", "prediction_module.py"))
    refmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(refmod)
    from mnk.predictor import PredictionModule
    torch.manual_seed(8)
    ours = PredictionModule(num_kp=4, kp_variance="matrix", num_features=40, dropout=0)
    torch.manual_seed(8)
    theirs = refmod.PredictionModule(num_kp=4, kp_variance="matrix", num_features=40, dropout=0)
    for (n, p), (m, q) in zip(ours.state_dict().items(), theirs.state_dict().items()):
        assert n == m and torch.equal(p, q), n
    perturbed(theirs, 9)
    ours.load_state_dict(theirs.state_dict())
    theirs64 = theirs.double()
    kp = make_kp(3, 4, 4, True, 10)
    kp64 = {k: v.double().requires_grad_() for k, v in kp.items()}
    o64 = theirs64(kp64)
    _loss(o64, 5).backward()
    ours.to(be.device)
    kpn = {k: v.to(be.device).requires_grad_() for k, v in kp.items()}
    on = ours(kpn)
    _loss(on, 5).backward()
    be.sync()
    for k in o64:
        assert (on[k].detach().cpu().double() - o64[k]).abs().max() < 2e-5
    for (n, p), q in zip(ours.named_parameters(), theirs64.parameters()):
        assert (p.grad.cpu().double() - q.grad).abs().max() < 2e-5 * max(1.0, float(q.grad.abs().max())), n
    for k in kp:
        assert (kpn[k].grad.cpu().double() - kp64[k].grad).abs().max() < 2e-5


# ---- the switch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", ["1", None])
def test_native_prediction_switch(tmp_path, switch):
    """run_reference.py on a stand-in of the reference tree's layout: with MNK_NATIVE_PREDICTION=1 `modules.prediction_module`
    is mnk.predictor (ahead of the tree's own file); without the switch the stand-in is imported"""
    script = tmp_path / "probe.py"
    script.write_text("import modules.prediction_module as pm, sys\n"
                      "from modules.prediction_module import PredictionModule\n"
                      "import mnk.predictor\n"
                      "print(pm.__file__); print(PredictionModule is getattr(mnk.predictor, 'PredictionModule'))\n")
    (tmp_path / "modules").mkdir()
    (tmp_path / "modules" / "prediction_module.py").write_text("PredictionModule = 'stand-in'\n")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MNK_NATIVE_PREDICTION")}
    if switch is not None:
        env["MNK_NATIVE_PREDICTION"] = switch
    out = subprocess.run([sys.executable, os.path.join(ROOT, "monkey-net_amd", "run_reference.py"), str(script)],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    if switch == "1":
        assert "monkey-net_amd/mnk/predictor.py" in lines[0] and lines[1] == "True"
    else:
        assert str(tmp_path) in lines[0] and lines[1] == "False"
