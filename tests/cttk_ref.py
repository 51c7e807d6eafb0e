"""Reference side of the CTTK tests (tests/test_cttk.py): the three kernels of
libmgic_cttk.so restated literally in numpy (include/mgic_cttk.h gives every
expression with its order), and the loop of mg_ic_code_amd/cttk.py on one box
that is the whole periodic domain, on top of tests/momentum_periodic_ref.py
(exact FFT solves, pad_wrap).  Test infrastructure only.

Arrays are (nz, ny, nx), i fastest; a `_g` array covers the box grown by one.
"""
import numpy as np

from tests import momentum_periodic_ref as Q
from tests import momentum_ref as R

TWO_THIRDS = 2.0 / 3.0


class BadCells(Exception):
    def __init__(self, count, iteration):
        super().__init__(f"{count} cells with I < 0 on pass {iteration}")
        self.count, self.iteration = count, iteration


def _nb(f_g, d, s):
    """the valid box of f_g shifted by s along direction d (0 = x, the last axis)"""
    sl = [slice(1, -1)] * 3
    sl[2 - d] = slice(1 + s, f_g.shape[2 - d] - 1 + s)
    return f_g[tuple(sl)]


def grad(K_g, d, dx):
    """D_d K = h * (K(+e_d) - K(-e_d)), h = 0.5 / dx, over the valid box"""
    h = 0.5 / dx
    return h * (_nb(K_g, d, +1) - _nb(K_g, d, -1))


def kernel_K(I):
    """k_cttk_K: (K, bad) over the valid cells."""
    ok = I >= 0.0
    with np.errstate(invalid="ignore"):
        K = np.where(ok, -np.sqrt(np.where(ok, I, 0.0)), 0.0)
    return K, int(np.count_nonzero(~ok))


def kernel_source(psi, K_g, S, dx):
    """k_cttk_source: the three S_i + c * D_i, psi and S_i over the valid box."""
    p2 = psi * psi
    p6 = (p2 * p2) * p2
    c = TWO_THIRDS * p6
    return [S[d] + c * grad(K_g, d, dx) for d in range(3)]


def kernel_constraints(K_g, ham, mom, ham_abs, dx):
    """k_cttk_constraints: (ham, [mom_i], ham_abs) corrected."""
    K = R.valid(K_g)
    t = TWO_THIRDS * (K * K)
    return (ham + t, [mom[d] - TWO_THIRDS * grad(K_g, d, dx) for d in range(3)],
            ham_abs + np.abs(t))


def corrected_constraints(bh, lo, hi, dx, psi_g, phi_g, pot, pi, LW_g, K):
    """The constraints at constant_K = 0 with the correction: dict(ham,
    ham_abs, mom)."""
    out = R.constraints(bh, lo, hi, dx, psi_g, phi_g, pot, pi, LW_g)
    ham, mom, ham_abs = kernel_constraints(Q.pad_wrap(K), out["ham"], out["mom"], out["ham_abs"],
                                           dx)
    return dict(ham=ham, ham_abs=ham_abs, mom=mom)


def cttk_loop(prm, n, phi_g, pot, pi, psi=None, tol=1e-10, max_iterations=50):
    """cttk.cttk_solve on one n^3 box: dict(K, LW_g, k_steps, k_max, k_mean,
    min_I (per evaluation of K), nets, nets_relative, iterations, converged,
    first (the constraints of the first pass's data: its K, no LW) and final
    (of the returned data))."""
    lo, hi, dx = (0, 0, 0), (n - 1,) * 3, prm.domainLength[0] / n
    bh = prm.bh(constant_K=0.0)
    psi = np.ones((n, n, n)) if psi is None else psi
    psi_g = Q.pad_wrap(psi)
    LW_g = [np.zeros((n + 2,) * 3) for _ in range(6)]
    out = dict(k_steps=[], min_I=[], nets=[], nets_relative=[], iterations=0, converged=False)
    K = None
    for p in range(max_iterations + 1):
        I = R.nl_integrand(bh, lo, hi, dx, psi_g, phi_g, pot, pi, [R.valid(a) for a in LW_g])
        out["min_I"].append(float(I.min()))
        K_prev = K
        K, bad = kernel_K(I)
        if bad:
            raise BadCells(bad, p)
        if p == 0:
            out["first"] = corrected_constraints(bh, lo, hi, dx, psi_g, phi_g, pot, pi, LW_g, K)
        else:
            step = float(np.abs(K - K_prev).max())
            out["k_steps"].append(step)
            if step <= tol * float(np.abs(K).max()):
                out["converged"] = True
                break
        if p == max_iterations:
            break
        S, _ = R.source(bh, lo, hi, dx, psi, phi_g, pot, pi)
        S = kernel_source(psi, Q.pad_wrap(K), S, dx)
        V, net = zip(*[Q.solve_periodic(s, dx) for s in S])
        U, _ = Q.solve_periodic(R.div_rhs([Q.pad_wrap(v) for v in V], dx), dx)
        W = R.w(list(V), Q.pad_wrap(U), dx)
        LW_g = [Q.pad_wrap(x) for x in R.lw([Q.pad_wrap(x) for x in W], dx)]
        smax = [float(np.abs(s).max()) for s in S]
        out["nets"].append(list(net))
        out["nets_relative"].append([m / x if x != 0.0 else 0.0 for m, x in zip(net, smax)])
        out["iterations"] += 1
    out.update(K=K, LW_g=LW_g, k_max=float(np.abs(K).max()), k_mean=Q.mean(K),
               final=corrected_constraints(bh, lo, hi, dx, psi_g, phi_g, pot, pi, LW_g, K))
    return out
