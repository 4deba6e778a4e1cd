"""Host emulation, in fp32 and in the documented order, of the split-K weight-gradient folds (csrc/conv_gemm.hip:
wgrad_reduce_kernel, csrc/dwconv.hip: dw_wgrad_reduce_kernel).  numpy float32 additions are single IEEE additions, so a fold
that keeps the order equals these bit for bit.

Dense fold.  An element is summed by SL split lanes.  Lane sl takes the slabs k = sl, sl + SL, ... in ascending order: while
four whole rounds remain (k + 3 SL < nsplit) it adds slab[k + i SL] onto the running sum s_i (i = 0..3); what is left goes
onto s_0; the lane's sum is (s_0 + s_1) + (s_2 + s_3).  The lanes are added in ascending order, lane 0 first.  SL follows from
the slab's shape alone (split_lanes).  With `accumulate` the result is grad + sum.

Depth-wise fold.  Eight lanes; lane sl adds the slabs b = sl, sl + 8, ... in ascending order onto one running sum; the lanes
are added in ascending order."""
import numpy as np

F = np.float32


def split_lanes(n, nsplit):
    """SL of a slab of n = Cout * taps * Cin_g elements in nsplit splits (launch_wgrad_reduce)"""
    if n <= 65536 and nsplit >= 64:
        return 16
    if n <= 1048576 and nsplit >= 32:
        return 8
    return 2 if nsplit >= 8 else 1


def fold_sum(slab, SL):
    """slab (nsplit, n) fp32 -> (n,) fp32"""
    nsplit, n = slab.shape
    assert slab.dtype == F
    lanes = []
    for sl in range(SL):
        s = [np.zeros(n, F) for _ in range(4)]
        k = sl
        while k + 3 * SL < nsplit:
            for i in range(4):
                s[i] = s[i] + slab[k + i * SL]
            k += 4 * SL
        while k < nsplit:
            s[0] = s[0] + slab[k]
            k += SL
        lanes.append((s[0] + s[1]) + (s[2] + s[3]))
    tot = lanes[0]
    for lane in lanes[1:]:
        tot = tot + lane
    return tot


def wgrad_fold(slab, cg_real, grad=None):
    """slab (nsplit, Cout, taps, Cin_g) fp32 -> OIHW gradient (Cout, cg_real, taps) fp32; grad: what it is accumulated onto"""
    nsplit, cout, taps, cg = slab.shape
    s = fold_sum(np.ascontiguousarray(slab).reshape(nsplit, -1), split_lanes(cout * taps * cg, nsplit)).reshape(cout, taps, cg)
    out = np.ascontiguousarray(s[:, :, :cg_real].transpose(0, 2, 1))
    return out if grad is None else grad.astype(F) + out


def dw_fold(slab, grad=None):
    """slab (nblk, taps, C) fp32 -> (C, taps) fp32"""
    nblk, taps, c = slab.shape
    assert slab.dtype == F
    flat = np.ascontiguousarray(slab).reshape(nblk, -1)
    lanes = []
    for sl in range(8):
        s = np.zeros(taps * c, F)
        for b in range(sl, nblk, 8):
            s = s + flat[b]
        lanes.append(s)
    tot = lanes[0]
    for lane in lanes[1:]:
        tot = tot + lane
    out = np.ascontiguousarray(tot.reshape(taps, c).T)
    return out if grad is None else grad.astype(F) + out
