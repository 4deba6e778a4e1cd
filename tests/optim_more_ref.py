"""Host references for the optimizer kernels added beside mt_sgd / mt_adamw (csrc/optim.hip: mt_step_scalars_kernel, mt_update_kernel<Adam,
Adamax, NAdam, RAdam, RMSprop>, mt_sgd_tab_kernel), written from torch.optim's single-tensor rules; nothing here calls the code under test.

As stem_optim_ref.py: every update takes and returns numpy arrays of dtype `dt` - np.float32 restates the kernel with ONE float32
operation per kernel operation in the kernel's order (the build uses -ffp-contract=off and the kernels are element-wise, so the device is
held to bit equality), np.float64 is the same rule in double.  Hyper-parameters are converted to fp32 first, as the kernels receive
them; the step scalars are taken as given (`scal`: the 16-entry array of step_scalars_f32, or step_scalars_f64's unrounded doubles).
tests/test_optim_more_ref_host.py pins every function against torch.optim on the CPU."""
import math

import numpy as np

from stem_optim_ref import U, sgd_f32, sgd_f64  # noqa: F401  (mt_sgd_tab_kernel is mt_sgd_kernel's rule with a per-tensor momentum)

F = np.float32
NSCAL = 16
BC1, BC2, BC1_SQRT, BC2_SQRT, MU, MU_NEXT, MU_PROD, MU_PROD_NEXT, RHO, RECT_ON, RECT, T, NADAM_G, NADAM_M = range(14)
ADAM, ADAMAX, NADAM, RADAM, RMSPROP = range(5)
NAMES = {ADAM: "Adam", ADAMAX: "Adamax", NADAM: "NAdam", RADAM: "RAdam", RMSPROP: "RMSprop"}

# ------------------------------------------------------------------------------------------------------------------ step scalars


def step_scalars_f64(beta1, beta2, t, mu_product_prev=1.0, momentum_decay=4e-3, state_dt=F):
    """mt_step_scalars_kernel in float64, NOT rounded: betas as the fp32 values the kernels get; `mu_product_prev` is the fp32 state
    before this step (ignored at t = 1, where the product starts from 1).  The one rounding inside: mu_product is fp32 STATE, so the
    new product is rounded to fp32 before 1 - mu_product and mu_product * mu_next are formed from it (as torch forms them from its
    fp32 `mu_product` tensor).  state_dt=np.float64 drops that rounding: the rule with a float64 state, as torch runs it in float64"""
    b1, b2, t = float(F(beta1)), float(F(beta2)), float(t)
    s = np.zeros(NSCAL, dtype=np.float64)
    p2 = b2 ** t
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - p2
    s[BC1], s[BC2], s[BC1_SQRT], s[BC2_SQRT] = bc1, bc2, math.sqrt(bc1), math.sqrt(bc2)
    mu = b1 * (1.0 - 0.5 * 0.96 ** (t * momentum_decay))
    mu_next = b1 * (1.0 - 0.5 * 0.96 ** ((t + 1.0) * momentum_decay))
    mp_exact = (1.0 if t == 1.0 else float(state_dt(mu_product_prev))) * mu
    mp = float(state_dt(mp_exact))
    mp_next = mp * mu_next
    s[MU], s[MU_NEXT], s[MU_PROD], s[MU_PROD_NEXT] = mu, mu_next, mp_exact, mp_next
    s[NADAM_G], s[NADAM_M] = (1.0 - mu) / (1.0 - mp), mu_next / (1.0 - mp_next)
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    rho = rho_inf - 2.0 * t * p2 / bc2
    on = rho > 5.0
    s[RHO], s[RECT_ON] = rho, 1.0 if on else 0.0
    s[RECT] = math.sqrt((rho - 4.0) * (rho - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho)) if on else 0.0
    s[T] = t
    return s


def step_scalars_f32(*a, **k):
    """the device array: every entry of step_scalars_f64 rounded once to fp32"""
    return step_scalars_f64(*a, **k).astype(F)


# ----------------------------------------------------------------------------------------------------------------------- updates


def _grad(dt, p, g, wd, coef):
    """gv = g*c (+ wd*p when wd != 0): clipping, then torch's coupled decay grad.add(param, alpha=weight_decay)"""
    gv = g * dt(F(coef))
    wd = dt(F(wd))
    if wd != 0:
        gv = gv + wd * p
    return gv


def _update(dt, kind, p, g, a, b, lr, wd, beta1, beta2, eps, scal, coef=1.0, momentum=0.0):
    """optim.hip upd<KIND> -> (p, a, b).  a, b: exp_avg, exp_avg_sq (Adam, NAdam, RAdam); exp_avg, exp_inf (Adamax); square_avg,
    momentum_buffer (RMSprop: beta2 is alpha, beta1 and scal are not read, `momentum` is the tensor's table entry)"""
    p, g, a, b = p.astype(dt), g.astype(dt), a.astype(dt), b.astype(dt)
    lr, b1, b2, eps = (dt(F(x)) for x in (lr, beta1, beta2, eps))
    one = dt(1)
    w1, w2 = one - b1, one - b2
    gv = _grad(dt, p, g, wd, coef)
    if kind == RMSPROP:
        mom = dt(F(momentum))
        sq = a * b2 + w2 * gv * gv
        q = gv / (np.sqrt(sq) + eps)
        if mom > 0:
            bv = b * mom + q
            return p - lr * bv, sq, bv
        return p - lr * q, sq, b
    s = [dt(x) for x in scal]
    mv = a + w1 * (gv - a)
    if kind == ADAMAX:
        un = np.maximum(b * b2, np.abs(gv) + eps)
        return p - (lr / s[BC1]) * (mv / un), mv, un
    vv = b * b2 + w2 * gv * gv
    if kind == ADAM:
        return p - (lr / s[BC1]) * (mv / (np.sqrt(vv) / s[BC2_SQRT] + eps)), mv, vv
    if kind == NADAM:
        denom = np.sqrt(vv / s[BC2]) + eps
        p1 = p - (lr * s[NADAM_G]) * (gv / denom)
        return p1 - (lr * s[NADAM_M]) * (mv / denom), mv, vv
    assert kind == RADAM
    bce = mv / s[BC1]
    if s[RECT_ON] != 0:
        return p - ((bce * lr) * (s[BC2_SQRT] / (np.sqrt(vv) + eps))) * s[RECT], mv, vv
    return p - bce * lr, mv, vv


def _pair(kind):
    return (lambda *a, **k: _update(np.float32, kind, *a, **k)), (lambda *a, **k: _update(np.float64, kind, *a, **k))


adam_f32, adam_f64 = _pair(ADAM)
adamax_f32, adamax_f64 = _pair(ADAMAX)
nadam_f32, nadam_f64 = _pair(NADAM)
radam_f32, radam_f64 = _pair(RADAM)
rmsprop_f32, rmsprop_f64 = _pair(RMSPROP)
UPDATE_F32 = {ADAM: adam_f32, ADAMAX: adamax_f32, NADAM: nadam_f32, RADAM: radam_f32, RMSPROP: rmsprop_f32}
UPDATE_F64 = {ADAM: adam_f64, ADAMAX: adamax_f64, NADAM: nadam_f64, RADAM: radam_f64, RMSPROP: rmsprop_f64}

# ------------------------------------------------------------------------------------------------------------------------ bounds
# |fp32 result - *_f64| for ONE step from fp32 inputs and the SAME fp32 step scalars, from the operation count (u = 2^-24), derived the
# way stem_optim_ref.adamw_bound is.  Shared pieces:
#   E_g   gv = g*c: u|g c|; with decay the product wd*p: u|wd p|, and the sum: u|gv|           -> u (|g c| + |wd p| + |gv|)
#   tol_m mv = m + w1*(gv - m): w1 = 1-beta1 (u), the difference (u), the product (u): 3u w1 (|gv| + |m|); gv's own error w1 E_g;
#         the sum u|mv|                                                                          -> u|mv| + w1 (3u (|gv| + |m|) + E_g)
#   tol_v vv = v*beta2 + (w2*gv)*gv, all terms positive: w2 (u), two products (2u), v*beta2 (u), the sum (u): 5u vv; gv's error enters
#         twice: 2 w2 |gv| E_g                                                                   -> 5u vv + 2 w2 |gv| E_g
#   a root halves a relative error and adds its own u (sqrtf and the fp32 division are correctly rounded in this build).
# (1 + 2^-10) covers second order; 1e-45 keeps a bound of exactly zero from failing on equality of zeros.


def _rel(tol, x):
    return np.where(x > 0, tol / np.where(x > 0, x, 1.0), 0.0)


def _pieces(kind, p, g, a, b, lr, wd, beta1, beta2, eps, scal, coef, momentum):
    f = lambda x: np.float64(F(x))
    lr, wd, b1, b2, eps, c = (f(x) for x in (lr, wd, beta1, beta2, eps, coef))
    p64, g64, a64, b64 = (x.astype(np.float64) for x in (p, g, a, b))
    gc = np.abs(g64 * c)
    gv = g64 * c + (wd * p64 if wd != 0 else 0.0)
    e_g = U * (gc + np.abs(wd * p64) + np.abs(gv)) if wd != 0 else U * gc
    return lr, wd, b1, b2, eps, p64, a64, b64, np.abs(gv), e_g


def update_bound(kind, p, g, a, b, lr, wd, beta1, beta2, eps, scal, coef=1.0, momentum=0.0):
    """(tol_p, tol_a, tol_b) for UPDATE_F32[kind] against UPDATE_F64[kind] on the same arguments:
    Adam     T = (lr/bc1) * (mv / denom), denom = sqrt(vv)/bc2s + eps: rel(denom) <= rel(vv)/2 + 3u (root, division, sum); T adds the
             division, lr/bc1 and the product: |T| (rel(denom) + 3u) + (lr/bc1)/denom tol_m; the final difference u|p'|.
    Adamax   un = max(beta2 u, |gv| + eps): one rounding on either arm and gv's error (max is 1-Lipschitz): u un + E_g.
             T = (lr/bc1) * (mv / un): |T| (tol_u/un + 3u) + (lr/bc1)/un tol_m; u|p'|.
    NAdam    denom = sqrt(vv/bc2) + eps: rel <= (rel(vv) + u)/2 + 2u.  T1 = (lr G) * (gv / denom), T2 = (lr M) * (mv / denom), each
             |T| (rel(denom) + 3u) plus its numerator's error over denom; two differences: u (|p1| + |p'|).
    RAdam    bce = mv/bc1 (u), * lr (u); unrectified: 2u|T| + lr/bc1 tol_m + u|p'|.  Rectified: A = bc2s / (sqrt(vv) + eps): rel <=
             rel(vv)/2 + 3u (root, sum, division); the products with A and rect 2u: |T| (rel(vv)/2 + 7u) + (lr/bc1) A rect tol_m + u|p'|.
    RMSprop  sq as vv with alpha: tol_sq.  q = gv / (sqrt(sq) + eps): |q| (rel(sq)/2 + 3u) + E_g / avg.  With momentum buf' = buf*mom + q:
             u|buf mom| + tol_q + u|buf'|; p' = p - lr buf': u|lr buf'| + lr tol_buf + u|p'|.  Without: u|lr q| + lr tol_q + u|p'|, the
             buffer is not written (bound 0)."""
    lr, wd, b1, b2, eps, p64, a64, b64, gv, e_g = _pieces(kind, p, g, a, b, lr, wd, beta1, beta2, eps, scal, coef, momentum)
    pn, an, bn = UPDATE_F64[kind](p, g, a, b, lr, wd, b1, b2, eps, scal, coef, momentum)
    s2 = 1 + 2.0 ** -10
    fin = lambda *t: tuple(x * s2 + 1e-45 for x in t)
    w2 = 1 - b2
    if kind == RMSPROP:
        mom = np.float64(F(momentum))
        tol_sq = 5 * U * an + 2 * w2 * gv * e_g
        avg = np.sqrt(an) + eps
        q = gv / avg
        tol_q = q * (_rel(tol_sq, an) / 2 + 3 * U) + e_g / avg
        if mom > 0:
            tol_b = U * np.abs(b64 * mom) + tol_q + U * np.abs(bn)
            return fin(U * np.abs(lr * bn) + lr * tol_b + U * np.abs(pn), tol_sq, tol_b)
        return fin(U * np.abs(lr * q) + lr * tol_q + U * np.abs(pn), tol_sq, np.zeros_like(pn))
    sc = [np.float64(x) for x in scal]
    w1 = 1 - b1
    tol_m = U * np.abs(an) + w1 * (3 * U * (gv + np.abs(a64)) + e_g)
    if kind == ADAMAX:
        tol_u = U * bn + e_g
        k = lr / sc[BC1]
        T = np.abs(k * an / bn)
        return fin(U * np.abs(pn) + T * (tol_u / bn + 3 * U) + k / bn * tol_m, tol_m, tol_u)
    tol_v = 5 * U * bn + 2 * w2 * gv * e_g
    rv = _rel(tol_v, bn)
    if kind == ADAM:
        k = lr / sc[BC1]
        denom = np.sqrt(bn) / sc[BC2_SQRT] + eps
        T = np.abs(k * an / denom)
        return fin(U * np.abs(pn) + T * (rv / 2 + 6 * U) + k / denom * tol_m, tol_m, tol_v)
    if kind == NADAM:
        denom = np.sqrt(bn / sc[BC2]) + eps
        rd = (rv + U) / 2 + 2 * U
        k1, k2 = lr * sc[NADAM_G], lr * sc[NADAM_M]
        T1, T2 = np.abs(k1 * gv / denom), np.abs(k2 * an / denom)
        p1 = np.abs(p64) + T1
        return fin(U * (p1 + np.abs(pn)) + (T1 + T2) * (rd + 3 * U) + k1 / denom * e_g + k2 / denom * tol_m, tol_m, tol_v)
    k = lr / sc[BC1]
    if sc[RECT_ON] != 0:
        A = sc[BC2_SQRT] / (np.sqrt(bn) + eps)
        T = np.abs(k * an * A * sc[RECT])
        return fin(U * np.abs(pn) + T * (rv / 2 + 7 * U) + k * A * sc[RECT] * tol_m, tol_m, tol_v)
    return fin(U * np.abs(pn) + 2 * U * np.abs(k * an) + k * tol_m, tol_m, tol_v)
