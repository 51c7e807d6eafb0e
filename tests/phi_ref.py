"""Reference side of the stored-phi_0 tests (tests/test_phi_field.py): the
profiles of MyPhiFunction.H and set_a_coef / set_rhs / set_constant_K_integrand
with phi_0 as a stored array, restated in numpy, and the oracle's nonlinear
loop fed by them.  Test infrastructure only.

Cell centres follow set_initial_conditions (SetLevelData.cpp:55-57):
loc = (iv + 0.5) dx - L/2, on the box grown by one ghost layer.  Arrays are
(nz, ny, nx), i fastest; `phi_g` / `psi_g` cover [lo - 1, hi + 1].
"""
import numpy as np

import oracle


def centres(lo, hi, dx, L, grow=1):
    """(x, y, z) broadcastable coordinate arrays over [lo - grow, hi + grow]."""
    ax = [(np.arange(lo[d] - grow, hi[d] + grow + 1, dtype=np.float64) + 0.5) * dx - L / 2.0
          for d in range(3)]
    return ax[0].reshape(1, 1, -1), ax[1].reshape(1, -1, 1), ax[2].reshape(-1, 1, 1)


def gaussian(bh, x, y, z):
    """MyPhiFunction.H:14-15."""
    r2 = x * x + y * y + z * z
    return bh["phi_amplitude"] * np.exp(-r2 / bh["phi_wavelength"])


def sine(bh, x, y, z):
    """MyPhiFunction.H:18-20 (the profile commented out beside the Gaussian)."""
    L, w = bh["domain_length"], bh["phi_wavelength"]
    return bh["phi_amplitude"] * (np.sin(2 * np.pi * x * w / L) + np.sin(2 * np.pi * y * w / L)
                                  + np.sin(2 * np.pi * z * w / L))


def phi_on_box(profile, bh, lo, hi, dx):
    """profile(bh, x, y, z) over the box grown by one, as a full array."""
    x, y, z = centres(lo, hi, dx, bh["domain_length"])
    shape = (z.size, y.size, x.size)
    return np.ascontiguousarray(np.broadcast_to(profile(bh, x, y, z), shape))


def _get_Aij(i, j, r1, r2, n1, n2, J1, J2, P1, P2):
    """get_Aij (SetBinaryBH.H:24-53), the loops as written."""
    eps = np.zeros((3, 3, 3))
    eps[0, 1, 2] = eps[1, 2, 0] = eps[2, 0, 1] = 1.0
    eps[0, 2, 1] = eps[2, 1, 0] = eps[1, 0, 2] = -1.0
    A = (1.5 / r1 / r1 * (n1[i] * P1[j] + n1[j] * P1[i])
         + 1.5 / r2 / r2 * (n2[i] * P2[j] + n2[j] * P2[i]))
    for k in range(3):
        A = A + (1.5 / r1 / r1 * (n1[i] * n1[j] - float(i == j)) * P1[k] * n1[k]
                 + 1.5 / r2 / r2 * (n2[i] * n2[j] - float(i == j)) * P2[k] * n2[k])
        for l in range(3):
            A = A + (-3.0 / r1 / r1 / r1 * (eps[i, l, k] * n1[j] + eps[j, l, k] * n1[i]) * n1[l]
                     * J1[k]
                     - 3.0 / r2 / r2 / r2 * (eps[i, l, k] * n2[j] + eps[j, l, k] * n2[i]) * n2[l]
                     * J2[k])
    return A


def bowen_york(bh, lo, hi, dx):
    """(A2, psi_bh) over [lo, hi]: A_ij_0 of set_binary_bh_Aij (SetBinaryBH.H:55-83)
    contracted as SetLevelData.cpp:312-317, and set_binary_bh_psi (SetBinaryBH.H:85-99)."""
    x, y, z = centres(lo, hi, dx, bh["domain_length"], grow=0)
    shape = (z.size, y.size, x.size)
    x, y, z = (np.broadcast_to(v, shape) for v in (x, y, z))
    l1, l2 = (x - bh["bh1_offset"], y, z), (x - bh["bh2_offset"], y, z)   # get_bh_radius, :15-20
    r1 = np.sqrt(l1[0] * l1[0] + l1[1] * l1[1] + l1[2] * l1[2])
    r2 = np.sqrt(l2[0] * l2[0] + l2[1] * l2[1] + l2[2] * l2[2])
    n1, n2 = [v / r1 for v in l1], [v / r2 for v in l2]                   # :65-68
    J1, J2 = (0.0, 0.0, bh["bh1_spin"]), (0.0, 0.0, bh["bh2_spin"])       # :71-74
    P1, P2 = (0.0, bh["bh1_momentum"], 0.0), (0.0, bh["bh2_momentum"], 0.0)
    A = {ij: _get_Aij(ij[0], ij[1], r1, r2, n1, n2, J1, J2, P1, P2)
         for ij in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))}
    A2 = (A[0, 0] ** 2.0 + A[1, 1] ** 2.0 + A[2, 2] ** 2.0 + 2 * A[0, 1] ** 2.0
          + 2 * A[0, 2] ** 2.0 + 2 * A[1, 2] ** 2.0)
    psi_bh = bh["bh1_bare_mass"] / r1 + bh["bh2_bare_mass"] / r2
    return A2, psi_bh


def _common(bh, lo, hi, dx, psi_g, phi_g, K):
    shape = tuple(hi[d] - lo[d] + 1 for d in (2, 1, 0))
    if psi_g is None:
        psi_g = np.ones(tuple(s + 2 for s in shape))
    assert psi_g.shape == phi_g.shape == tuple(s + 2 for s in shape)
    lap = oracle.getlaplacianpsif(psi_g, lo, hi, dx)        # SetLevelDataF.ChF:15-58
    rho_grad = oracle.getrhogradphif(phi_g, lo, hi, dx)     # SetLevelDataF.ChF:65-103
    A2, psi_bh = bowen_york(bh, lo, hi, dx)
    rho = 0.0                                               # V = 0, Pi = 0 (set_m_value)
    m = (2.0 / 3.0) * (K * K) - 16.0 * np.pi * bh["G_Newton"] * rho
    psi_0 = psi_g[1:-1, 1:-1, 1:-1] + psi_bh                # SetLevelData.cpp:118-119
    return lap, rho_grad, A2, m, psi_0


def nl_coefs_phi(bh, lo, hi, dx, psi_g, phi_g):
    """(aCoef, rhs): set_a_coef (SetLevelData.cpp:281-325) and set_rhs (:73-127)
    with c_phi_0 = phi_g; psi_g None: psi = 1."""
    lap, rho_grad, A2, m, psi_0 = _common(bh, lo, hi, dx, psi_g, phi_g, bh["constant_K"])
    G = bh["G_Newton"]
    a = -0.625 * m * psi_0 ** 4.0 - A2 * psi_0 ** -8.0 + 2.0 * np.pi * G * rho_grad   # :321-322
    r = (0.125 * m * psi_0 ** 5.0 - 0.125 * A2 * psi_0 ** -7.0
         - 2.0 * np.pi * G * rho_grad * psi_0 - lap)                                    # :121-124
    return a, r


def nl_integrand_phi(bh, lo, hi, dx, psi_g, phi_g):
    """set_constant_K_integrand (SetLevelData.cpp:131-180; m at K = 0, :167)."""
    lap, rho_grad, A2, m, psi_0 = _common(bh, lo, hi, dx, psi_g, phi_g, 0.0)
    return (-1.5 * m + 1.5 * A2 * psi_0 ** -12.0
            + 24.0 * np.pi * bh["G_Newton"] * rho_grad * psi_0 ** -4.0
            + 12.0 * lap * psi_0 ** -5.0)                                               # :181-184


def oracle_poisson_solve_phi(prm, n, max_depth, n_nl, phi_g, bottom_solver=1, perturb=None):
    """tests/nl_ref.oracle_poisson_solve on one periodic or Dirichlet n^3 box
    with the coefficients of the restatement above (stored phi_0 = phi_g).
    perturb: an array of relative perturbations applied to aCoef and rhs
    (the sensitivity check of the iteration counts)."""
    dom = (0, 0, 0, n - 1, n - 1, n - 1)
    lo, hi = dom[:3], dom[3:]
    dx = prm.domainLength[0] / n
    bh = prm.bh(constant_K=0.0)
    avg = prm.coefficient_average_type if prm.coefficient_average_type >= 0 else 0
    per = (1, 1, 1) if prm.is_periodic else (0, 0, 0)
    volume = prm.domainLength[0] * prm.domainLength[1] * prm.domainLength[2]
    o = oracle.OracleMG([dom], dom, dx, alpha=prm.alpha, beta=prm.beta, periodic=per,
                        bc_lo=prm.bc_lo, bc_hi=prm.bc_hi, bc_value=prm.bc_value,
                        nlevels=max_depth + 1, avg_type=avg, prolong_type=1,
                        bottom_solver=bottom_solver, n_pre=prm.numMGsmooth,
                        n_post=prm.numMGsmooth, n_bottom=prm.numMGsmooth)
    psi = np.ones((n + 2,) * 3)
    o.set(0, oracle.PHI, 0, np.zeros((n,) * 3))
    norms, iters, ks = [], [], []
    for _ in range(n_nl):
        if prm.is_periodic:  # Main_PoissonSolver.cpp:133-147
            bh["constant_K"] = 0.0
            integ = nl_integrand_phi(bh, lo, hi, dx, psi, phi_g)
            bh["constant_K"] = -np.sqrt(abs(np.sum(integ) * dx ** 3) / volume)
            ks.append(bh["constant_K"])
        a, r = nl_coefs_phi(bh, lo, hi, dx, psi, phi_g)
        if perturb is not None:
            a, r = a * (1.0 + perturb), r * (1.0 - perturb)
        o.set(0, oracle.ACOEF, 0, a)
        o.set(0, oracle.BCOEF, 0, np.ones_like(a))
        o.set(0, oracle.RHS, 0, r)
        o.setup()
        it, _ = o.solve(mg_iters=prm.numMGIterations, imax=prm.max_iterations,
                        eps=prm.tolerance, norm_type=0)
        iters.append(it)
        o.exchange(0, oracle.PHI)          # set_update_psi0
        o.fill_bc(0, oracle.PHI, 0)
        psi += o.get(0, oracle.PHI, 0, full=True)
        dpsi = o.get(0, oracle.PHI, 0)
        nrm = np.sqrt(np.sum(dpsi * dpsi)) * dx ** 1.5
        norms.append(nrm)
        if nrm < prm.tolerance or nrm > 1e5:
            break
    return psi, norms, iters, ks
