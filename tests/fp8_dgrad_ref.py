"""Restatements shared by the fp8 data-gradient tests (host and GPU): the weight layout of the swapped problem and its meaning.

The data gradient of a 3x3, stride 1, pad 1 convolution y = conv(x, w) is dx[ci, q] = sum_{co, t} dy[co, q - d(t)] * w[co, ci, t] with
d(t) = (t // 3 - 1, t % 3 - 1); d(8 - t) = -d(t), so dx[ci, q] = sum_{co, t'} dy[co, q + d(t')] * w[co, ci, 8 - t']: a 3x3 "same" convolution
of dy whose "output channel" is ci, whose reduction runs over co, and whose tap t' holds w[.., 8 - t']."""
import numpy as np
import torch


def pack_dgrad_ref(codes, groups=1, lo=0, hi=None):
    """codes (Cout, Cin / groups, 3, 3) -> [groups][Cin / groups][9 taps, flipped][(hi - lo) / groups]: y3d_fp8_pack_weight_dgrad's layout for
    the output channels [lo, hi) (a window needs groups == 1)"""
    codes = np.asarray(codes)
    Cout, Cig = codes.shape[:2]
    hi = Cout if hi is None else hi
    assert groups == 1 or (lo, hi) == (0, Cout)
    c = codes.reshape(groups, Cout // groups, Cig, 9)
    if groups == 1:
        c = c[:, lo:hi]
    c = c[:, :, :, ::-1]                         # tap t' <- tap 8 - t'
    return np.ascontiguousarray(c.transpose(0, 2, 3, 1))


def multiply_out(dy, packed):
    """dy (B, Cw, H, W) float64 (the window's channels), packed [G][Cig][9][Cwg] VALUES -> dx (B, G * Cig, H, W): the packed layout read as
    the weights of a 3x3 'same' convolution of dy, tap t' at offset (t' // 3 - 1, t' % 3 - 1)"""
    G, Cig, _, Cwg = packed.shape
    w = torch.as_tensor(packed, dtype=torch.float64).permute(0, 1, 3, 2).reshape(G * Cig, Cwg, 3, 3)
    return torch.nn.functional.conv2d(dy.double(), w, None, 1, 1, 1, G)


def e4m3_value(codes):
    """uint8 e4m3fn codes -> float64 values"""
    return torch.as_tensor(np.asarray(codes)).contiguous().view(torch.float8_e4m3fn).double()
