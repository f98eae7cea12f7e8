"""Helpers shared by the kernel tests."""
import torch


def ceil4(c):
    return (c + 3) // 4 * 4


def to_nhwc(x4, ld=None, pad_value=0.0):
    """(N,C,H,W) -> (N,H,W,ld) with pad channels = pad_value."""
    n, c, h, w = x4.shape
    ld = ld or ceil4(c)
    out = torch.full((n, h, w, ld), pad_value, dtype=x4.dtype)
    out[..., :c] = x4.permute(0, 2, 3, 1)
    return out


def from_nhwc(x, c):
    return x[..., :c].permute(0, 3, 1, 2).contiguous()


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def maxerr(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def within(label, metric, got, ref64, ref32, project):
    """A measured tolerance: `got` must lie within max(project, 4 * e_ref) of the fp64 reference, where
    e_ref = metric(ref32, ref64) is the error of the SAME reference computed in fp32 by stock torch on the CPU -- the rounding
    that the arithmetic itself costs at this shape.  The factor 4: the kernel and ATen round the same coordinate arithmetic in
    another order (fused multiply-adds on the device), errors of one kind but not equal.  ref32 None: the project bound alone.
    The figures are printed before anything is asserted (`pytest -s` shows them); returns (ok, error, e_ref)."""
    err = metric(got, ref64)
    e_ref = metric(ref32, ref64) if ref32 is not None else None
    bound = project if e_ref is None else max(project, 4 * e_ref)
    print("FIGURE %s: error %.3e fp32-reference %s bound %.3e" % (label, err, "%.3e" % e_ref if e_ref is not None else "-", bound))
    return err < bound, err, e_ref


def set_library(path, strict=True):
    """TEST INFRASTRUCTURE: bind the C-ABI of another build of the same kernel sources (the CPU emulator build used by the
    `-m "not gpu"` tests) by replacing the product's process-wide library handle; None: back to the in-tree gfx950 build on
    next use.  The product has no such switch (its only library override is the MNK_LIBRARY path)."""
    from mnk import _lib
    _lib._LIB = _lib.Library(path, strict=strict) if path is not None else None
    return _lib._LIB
