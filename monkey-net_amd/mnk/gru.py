"""torch.autograd wrappers around the GRU kernels of libmonkeynet_hip.so (csrc/gru.hip): one nn.GRU layer (batch_first), the
output head's nn.Linear and the head of modules/prediction_module.py:33-42 (mean = tanh, var = V^T V).  Used by
mnk.predictor.PredictionModule; kept out of mnk/ops.py.

Internal layouts (time-major, so that a step's rows are one contiguous block):
  Gi, dGi, dGh  [T, B, 3H]       hs  [T + 1, B, H]: hs[0] = h0, hs[t + 1] = h_t        gates  [T, B, 4H] = r | z | n | hn
The layer's output is the view hs[1:].transpose(0, 1) ([B, T, H]); every GEMM reads such views through grouped rows
(include/monkeynet_hip.h), so a non-contiguous input (a slice of a key-point tensor) is read where it lies.
PyTorch is used for memory, streams and the autograd tape only; every arithmetic step is a kernel launch."""
import torch

from . import ops
from .ops import _Fn, _call, _query, _p


def _rows(t):
    """(ld, grp, ld_grp) of the rows of a 2-D tensor or of the (dim 0, dim 1) rows of a 3-D tensor; the last stride must be 1."""
    assert t.stride(-1) == 1 or t.shape[-1] <= 1, "GRU operands need a unit stride along their last dimension"
    if t.dim() == 2:
        return t.stride(0), 0, 0
    return t.stride(1), t.shape[1], t.stride(0)


def _unit(t):
    return t if t.stride(-1) == 1 or t.shape[-1] <= 1 else t.contiguous()


def gemm(transA, transB, M, N, K, A, B, C, bias=None):
    """C[M, N] = op(A) op(B) (+ bias): A is a [M, K] (transA=0) or [K, M] (1) matrix, B [K, N] (transB=0) or [N, K] (1); either may
    be a 3-D tensor whose first two dimensions are its rows.  C is a plain row-major [M, N] (a 2-D or 3-D contiguous tensor)."""
    ws_n = _query("mnk_gru_gemm_workspace_floats", M, N, K)
    ws = torch.empty(ws_n, dtype=torch.float32, device=C.device) if ws_n else None
    lda, ag, ldag = _rows(A)
    ldb, bg, ldbg = _rows(B)
    _call("mnk_gru_gemm", C, transA, transB, M, N, K, _p(A), lda, ag, ldag, _p(B), ldb, bg, ldbg, _p(bias), _p(C), N, _p(ws),
          ws_n)
    return C


def colsum(x2d):
    rows, cols = x2d.shape
    ws_n = _query("mnk_gru_colsum_workspace_floats", rows, cols)
    ws = torch.empty(max(ws_n, 1), dtype=torch.float32, device=x2d.device)
    out = torch.empty(cols, dtype=torch.float32, device=x2d.device)
    _call("mnk_gru_colsum", x2d, _p(x2d), x2d.stride(0), rows, cols, _p(out), _p(ws), ws_n)
    return out


class GRULayerFn(_Fn):
    """One nn.GRU layer (batch_first): x [B, T, I] (any batch / time strides), h0 [B, H] or None -> (out [B, T, H], h_n [B, H]).
    Replaces torch.nn.GRU of modules/prediction_module.py:20 (one layer of it)."""

    @staticmethod
    def forward(ctx, x, h0, w_ih, w_hh, b_ih, b_hh):
        ops._check_device(x)
        x = _unit(x)
        w_ih, w_hh, b_ih, b_hh = (p.contiguous() for p in (w_ih, w_hh, b_ih, b_hh))
        B, T, I = x.shape
        H = w_hh.shape[1]
        dev = x.device
        gi = torch.empty(T, B, 3 * H, dtype=torch.float32, device=dev)
        # rows (t, b) of x: b * stride(0) + t * stride(1)
        xt = x.transpose(0, 1)
        gemm(0, 1, T * B, 3 * H, I, xt, w_ih, gi, b_ih)
        hs = torch.empty(T + 1, B, H, dtype=torch.float32, device=dev)
        if h0 is None:
            hs[0].zero_()
        else:
            hs[0].copy_(h0)
        train = any(ctx.needs_input_grad)
        gates = torch.empty(T, B, 4 * H, dtype=torch.float32, device=dev) if train else None
        for t in range(T):
            _call("mnk_gru_step_fwd", x, _p(hs[t]), H, _p(w_hh), _p(b_hh), _p(gi[t]), 3 * H, _p(hs[t + 1]), H,
                  _p(gates[t]) if train else None, B, H)
        out = hs[1:].transpose(0, 1)
        h_n = hs[T].clone()
        if train:
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(x, w_ih, w_hh, hs, gates)
            ctx.h0_given = h0 is not None
        return out, h_n

    @staticmethod
    def backward(ctx, dout, dhn):
        x, w_ih, w_hh, hs, gates = ctx.saved_tensors
        B, T, I = x.shape
        H = w_hh.shape[1]
        dev = x.device
        if dout is not None:
            dout = dout.contiguous()
        dhn = None if dhn is None else dhn.contiguous()
        ld_dy = T * H
        dgi = torch.empty(T, B, 3 * H, dtype=torch.float32, device=dev)
        dgh = torch.empty(T, B, 3 * H, dtype=torch.float32, device=dev)
        carry = torch.empty(B, H, dtype=torch.float32, device=dev)
        dy = (lambda t: None) if dout is None else (lambda t: _p(dout[:, t]))
        _call("mnk_gru_gates_bwd", x, dy(T - 1), ld_dy, _p(dhn), _p(gates[T - 1]), _p(hs[T - 1]), H, _p(dgi[T - 1]), _p(dgh[T - 1]),
              _p(carry), B, H)
        for t in range(T - 1, 0, -1):
            _call("mnk_gru_step_bwd", x, _p(dgh[t]), _p(w_hh), _p(carry), dy(t - 1), ld_dy, _p(gates[t - 1]), _p(hs[t - 1]), H,
                  _p(dgi[t - 1]), _p(dgh[t - 1]), None, H, B, H)
        need = ctx.needs_input_grad
        dx = dh0 = dw_ih = dw_hh = db_ih = db_hh = None
        if need[1] and ctx.h0_given:
            dh0 = torch.empty(B, H, dtype=torch.float32, device=dev)
            _call("mnk_gru_step_bwd", x, _p(dgh[0]), _p(w_hh), _p(carry), None, 0, None, None, 0, None, None, _p(dh0), H, B, H)
        if need[0]:
            dxt = torch.empty(T, B, I, dtype=torch.float32, device=dev)
            gemm(0, 0, T * B, I, 3 * H, dgi, w_ih, dxt)
            dx = dxt.transpose(0, 1)
        if need[2]:
            dw_ih = gemm(1, 0, 3 * H, I, T * B, dgi, x.transpose(0, 1), torch.empty(3 * H, I, dtype=torch.float32, device=dev))
        if need[3]:
            dw_hh = gemm(1, 0, 3 * H, H, T * B, dgh, hs[:T], torch.empty(3 * H, H, dtype=torch.float32, device=dev))
        if need[4]:
            db_ih = colsum(dgi.view(T * B, 3 * H))
        if need[5]:
            db_hh = colsum(dgh.view(T * B, 3 * H))
        return dx, dh0, dw_ih, dw_hh, db_ih, db_hh


class LinearFn(_Fn):
    """y [B, T, N] = x [B, T, K] W^T + b (nn.Linear of modules/prediction_module.py:23 over the GRU's output rows)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ops._check_device(x)
        x = _unit(x)
        w, b = w.contiguous(), b.contiguous()
        Bn, T, K = x.shape
        N = w.shape[0]
        y = torch.empty(Bn, T, N, dtype=torch.float32, device=x.device)
        gemm(0, 1, Bn * T, N, K, x, w, y, b)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        Bn, T, K = x.shape
        N = w.shape[0]
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = gemm(0, 0, Bn * T, K, N, dy, w, torch.empty(Bn, T, K, dtype=torch.float32, device=dy.device))
        if ctx.needs_input_grad[1]:
            dw = gemm(1, 0, N, K, Bn * T, dy, x, torch.empty(N, K, dtype=torch.float32, device=dy.device))
        if ctx.needs_input_grad[2]:
            db = colsum(dy.view(Bn * T, N))
        return dx, dw, db


class HeadFn(_Fn):
    """modules/prediction_module.py:33-42: y [B, T, num_kp * F] -> mean [B, T, num_kp, 2] = tanh(y[..., :2]) and, with has_var,
    var [B, T, num_kp, 2, 2] = V^T V (V = y[..., 2:6] as 2 x 2)."""

    @staticmethod
    def forward(ctx, y, num_kp, has_var):
        ops._check_device(y)
        y = y.contiguous()
        Bn, T, N = y.shape
        F = N // num_kp
        mean = torch.empty(Bn, T, num_kp, 2, dtype=torch.float32, device=y.device)
        var = torch.empty(Bn, T, num_kp, 2, 2, dtype=torch.float32, device=y.device) if has_var else None
        _call("mnk_gru_head_fwd", y, _p(y), Bn * T, num_kp, F, int(has_var), _p(mean), _p(var))
        if ctx.needs_input_grad[0]:
            ctx.set_materialize_grads(False)
            ctx.save_for_backward(y)
            ctx.meta = (num_kp, F, has_var)
        return (mean, var) if has_var else mean

    @staticmethod
    def backward(ctx, dmean, dvar=None):
        (y,) = ctx.saved_tensors
        num_kp, F, has_var = ctx.meta
        dmean = None if dmean is None else dmean.contiguous()
        dvar = None if dvar is None else dvar.contiguous()
        dy = torch.empty_like(y)
        _call("mnk_gru_head_bwd", y, _p(y), _p(dmean), _p(dvar), y.shape[0] * y.shape[1], num_kp, F, int(has_var), _p(dy))
        return dy, None, None
