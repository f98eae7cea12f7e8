"""fp64 restatement of the transfer-time key-point normalisation (transfer.py:31-62 normalize_kp with make_symetric_matrix,
transfer.py:17-28) in torch + numpy, shared by the tests of mnk.engine.Transfer and of the mnk_kp_normalize kernel."""
import numpy as np
import torch


def normalize_kp_fp64(mv, vv, ma, va, mult=1.0, move_location=True, clip_mean=True, adapt_variance=True):
    """mv (B,D,K,2) / vv (B,D,K,2,2): the driving video's key points, ma (B,1,K,2) / va (B,1,K,2,2): the source's, all fp64;
    mult = sqrt(hull area of ma[0, 0]) / sqrt(hull area of mv[0, 0]) under movement_mult, else 1.  -> (mean, var)"""
    from modules.util import matrix_inverse
    mean, var = mv, vv
    if move_location:
        mean = (mv - mv[:, 0:1]) * mult + ma
    if clip_mean:
        mean = mean.clamp(-1, 1)
    if adapt_variance:
        var = torch.matmul(torch.matmul(vv, matrix_inverse(vv[:, 0:1])), va)
        sym = (var + var.transpose(-1, -2)) / 2
        ev, eu = np.linalg.eigh(sym.numpy())
        ev[ev <= 0] = 1e-6
        var = torch.from_numpy(np.einsum("...ij,...j,...kj->...ik", eu, ev, eu))
    return mean, var
