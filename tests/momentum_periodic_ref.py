"""Reference side of the periodic momentum-solve tests
(tests/test_momentum_periodic.py): the projected step of
mg_ic_code_amd/momentum.py on one periodic box, restated in numpy on top of
tests/momentum_ref.py.  Test infrastructure only.

What changes against the Dirichlet restatement:

    ghosts       every field is padded by wrapping (pad_wrap), in place of
                 momentum_ref.pad_extrap and pad_dirichlet
    the solves   the compact 7-point Laplacian inverted exactly by FFT with
                 the zero mode dropped (solve_periodic), in place of
                 solve_dirichlet: the mean of the right-hand side is removed
                 (and returned), and the solution has mean zero
    the NL loop  the oracle's periodic one, the momentum step in front of the
                 K integrand so that K = -sqrt(|sum integrand dV| / volume)
                 comes from the total tensor Abar^BY_ij + LW_ij

The mean is np.sum(f) / f.size; the device's is its own dotProduct(f, ones) /
cells, whose order of summation differs (see test_momentum_periodic.MEAN_ULPS).
Arrays are (nz, ny, nx), i fastest; a `_g` array covers the box grown by one.
"""
import numpy as np

from tests import momentum_ref as R
from tests import phi_ref


def pad_wrap(f):
    """f over a box that is the whole periodic domain -> over the box grown by
    one, every ghost (edges and corners too) the wrapped valid value."""
    return np.pad(f, 1, mode="wrap")


def mean(f):
    return float(np.sum(f) / f.size)


def laplacian(u, dx):
    """The compact 7-point Laplacian of u on the periodic box."""
    g = pad_wrap(u)
    out = -6.0 * u
    for ax in range(3):
        lo, hi = [slice(1, -1)] * 3, [slice(1, -1)] * 3
        lo[ax], hi[ax] = slice(0, -2), slice(2, None)
        out = out + g[tuple(lo)] + g[tuple(hi)]
    return out / dx ** 2


def solve_periodic(s, dx):
    """(u, m): m the mean of s, u the mean-zero solution of Lap u = s - m on
    the periodic box, the 7-point Laplacian inverted exactly by FFT."""
    lam = [(2.0 * np.cos(2.0 * np.pi * np.arange(n) / n) - 2.0) / dx ** 2 for n in s.shape]
    ev = lam[0][:, None, None] + lam[1][None, :, None] + lam[2][None, None, :]
    ev[0, 0, 0] = 1.0
    m = mean(s)
    hat = np.fft.fftn(s - m) / ev
    hat[0, 0, 0] = 0.0
    return np.real(np.fft.ifftn(hat)), m


def momentum_step(bh, lo, hi, dx, psi_g, phi_g, pot, pi, table=None):
    """The projected step of an NL iteration on one box that is the whole
    periodic domain: dict(S, net, net_relative, V, U, W, LW_g, u_mean): S the
    source as it comes, net the three means removed from it, net_relative each
    over max|S_i|, u_mean the mean removed from U's right-hand side, LW_g the
    six components with their wrapped ghosts."""
    S, _ = R.source(bh, lo, hi, dx, R.valid(psi_g), phi_g, pot, pi, table)
    V, net = zip(*[solve_periodic(s, dx) for s in S])
    U, u_mean = solve_periodic(R.div_rhs([pad_wrap(v) for v in V], dx), dx)
    W = R.w(list(V), pad_wrap(U), dx)
    LW = R.lw([pad_wrap(x) for x in W], dx)
    smax = [float(np.abs(s).max()) for s in S]
    return dict(S=S, net=list(net), net_relative=[m / x if x != 0.0 else 0.0
                                                  for m, x in zip(net, smax)],
                V=list(V), U=U, W=W, LW_g=[pad_wrap(x) for x in LW], u_mean=u_mean)


def coupled_solve(prm, n, max_depth, phi_g, pot, pi, momentum_on=True, table=None):
    """The oracle's periodic NL loop (phi_ref.oracle_poisson_solve_phi) on one
    n^3 box with the matter; with momentum_on the projected momentum step in
    front of every K integrand, K and the coefficients from the total tensor.
    Returns dict(psi_g, norms, iters, ks, nets, nets_relative, mom, mom_net,
    ham, ham_abs, LW_g): the constraints of the final psi with the final total
    tensor and the last K; mom_net[i] = Mom_i + m_i psi_0^-6, m the means of
    the last step."""
    lo, hi, dx = (0, 0, 0), (n - 1,) * 3, prm.domainLength[0] / n
    zeros = [np.zeros((n, n, n)) for _ in range(6)]
    state = {"nets": [], "rel": []}

    def integrand(bh, lo_, hi_, dx_, psi_g, phi_g_):
        if not momentum_on:
            return R.nl_integrand(bh, lo_, hi_, dx_, psi_g, phi_g_, pot, pi, zeros, table)
        step = momentum_step(bh, lo_, hi_, dx_, psi_g, phi_g_, pot, pi, table)
        state["LW_g"] = step["LW_g"]
        state["nets"].append(step["net"])
        state["rel"].append(step["net_relative"])
        return R.nl_integrand(bh, lo_, hi_, dx_, psi_g, phi_g_, pot, pi,
                              [R.valid(a) for a in step["LW_g"]], table)

    def coefs(bh, lo_, hi_, dx_, psi_g, phi_g_):
        abar = [R.valid(a) for a in state["LW_g"]] if momentum_on else zeros
        return R.nl_coefs(bh, lo_, hi_, dx_, psi_g, phi_g_, pot, pi, abar, table)

    saved = phi_ref.nl_coefs_phi, phi_ref.nl_integrand_phi
    phi_ref.nl_coefs_phi, phi_ref.nl_integrand_phi = coefs, integrand
    try:
        psi_g, norms, iters, ks = phi_ref.oracle_poisson_solve_phi(
            prm, n, max_depth, prm.max_NL_iterations, phi_g)
    finally:
        phi_ref.nl_coefs_phi, phi_ref.nl_integrand_phi = saved
    bh = prm.bh(constant_K=ks[-1])
    LW_g = state.get("LW_g", [np.zeros((n + 2,) * 3) for _ in range(6)])
    out = R.constraints(bh, lo, hi, dx, psi_g, phi_g, pot, pi, LW_g, table)
    net = state["nets"][-1] if state["nets"] else [0.0, 0.0, 0.0]
    # psi_0 = psi + psi_bh, as momentum_ref.momentum forms it
    from tests import constraints_ref as C
    from tests import puncture_ref as P
    _, psi_bh = P.bowen_york(C._table(bh, table), bh["domain_length"], lo, hi, dx)
    w = (R.valid(psi_g) + psi_bh) ** -6.0
    out.update(psi_g=psi_g, norms=norms, iters=iters, ks=ks, nets=state["nets"],
               nets_relative=state["rel"], LW_g=LW_g, psi6inv=w,
               mom_net=[m + c * w for m, c in zip(out["mom"], net)])
    return out
