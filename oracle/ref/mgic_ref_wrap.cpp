/*
 * mgic_ref_wrap.cpp -- a plain C face for the reference's level-data
 * functions, compiled from the reference's own Source/SetLevelData.cpp.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/reference.py binds it).  This file is
 * this project's code: it aliases caller arrays as FArrayBoxes over explicit
 * boxes (chombo_standin.H), fills the reference's own PoissonParameters
 * class from plain arguments and calls the reference's functions.  It
 * restates none of their arithmetic.  The ChomboFortran kernels need no
 * wrapper: the translated Fortran already has the C ABI of include/mgic_chf.h.
 */
#include "chombo_standin.H"

#include "PoissonParameters.H"
#include "SetLevelData.H"

/* defined in SetLevelData.cpp's object through the headers it includes */
Real get_Aij(const int, const int, const Real &, const Real &, const RealVect &, const RealVect &,
             const RealVect &, const RealVect &, const RealVect &, const RealVect &,
             const PoissonParameters &);
void set_binary_bh_Aij(FArrayBox &, const IntVect &, const RealVect &, const PoissonParameters &);
Real set_binary_bh_psi(const RealVect &, const PoissonParameters &);
Real my_phi_function(RealVect, Real, Real, RealVect);

extern "C" {

struct mgic_ref_params {
  double L[3]; /* domainLength */
  double G_Newton, phi_amplitude, phi_wavelength;
  double bh1_bare_mass, bh2_bare_mass, bh1_spin, bh2_spin;
  double bh1_momentum, bh2_momentum, bh1_offset, bh2_offset;
};

struct mgic_ref_fab {
  double *p;
  int lo[3], hi[3];
  int ncomp;
};

static int g_mayday = 0;
/* MayDay::Error / CH_assert: recorded, never fatal to the test process */
void mgic_ref_mayday(void) { ++g_mayday; }
void maydayerror_(void) { ++g_mayday; } /* call MAYDAYERROR() of the .ChF */
int mgic_ref_mayday_count(void) { return g_mayday; }
void mgic_ref_mayday_reset(void) { g_mayday = 0; }

} /* extern "C" */

namespace {

PoissonParameters params_of(const mgic_ref_params *q) {
  PoissonParameters p;
  p.domainLength = RealVect(q->L[0], q->L[1], q->L[2]);
  p.G_Newton = q->G_Newton;
  p.phi_amplitude = q->phi_amplitude;
  p.phi_wavelength = q->phi_wavelength;
  p.bh1_bare_mass = q->bh1_bare_mass;
  p.bh2_bare_mass = q->bh2_bare_mass;
  p.bh1_spin = q->bh1_spin;
  p.bh2_spin = q->bh2_spin;
  p.bh1_momentum = q->bh1_momentum;
  p.bh2_momentum = q->bh2_momentum;
  p.bh1_offset = q->bh1_offset;
  p.bh2_offset = q->bh2_offset;
  p.alpha = 1.0;
  p.beta = -1.0;
  return p;
}

Box box_of(const mgic_ref_fab *f) {
  return Box(IntVect(f->lo[0], f->lo[1], f->lo[2]), IntVect(f->hi[0], f->hi[1], f->hi[2]));
}

/* a one-box level over the caller's memory */
struct Level {
  FArrayBox fab;
  LevelData<FArrayBox> data;
  explicit Level(const mgic_ref_fab *f) : fab(box_of(f), f->ncomp, f->p), data(fab) {}
};

RealVect vec(const double *v) { return RealVect(v[0], v[1], v[2]); }

} // namespace

extern "C" {

void mgic_ref_set_initial_conditions(const mgic_ref_params *q, mgic_ref_fab *multigrid_vars,
                                     mgic_ref_fab *dpsi, double dx) {
  Level mv(multigrid_vars), dp(dpsi);
  set_initial_conditions(mv.data, dp.data, RealVect(dx, dx, dx), params_of(q));
}

void mgic_ref_set_rhs(const mgic_ref_params *q, mgic_ref_fab *rhs, mgic_ref_fab *multigrid_vars,
                      double dx, double constant_K) {
  Level r(rhs), mv(multigrid_vars);
  set_rhs(r.data, mv.data, RealVect(dx, dx, dx), params_of(q), constant_K);
}

void mgic_ref_set_a_coef(const mgic_ref_params *q, mgic_ref_fab *acoef,
                         mgic_ref_fab *multigrid_vars, double dx, double constant_K) {
  Level a(acoef), mv(multigrid_vars);
  set_a_coef(a.data, mv.data, params_of(q), RealVect(dx, dx, dx), constant_K);
}

void mgic_ref_set_b_coef(const mgic_ref_params *q, mgic_ref_fab *bcoef, double dx) {
  Level b(bcoef);
  set_b_coef(b.data, params_of(q), RealVect(dx, dx, dx));
}

void mgic_ref_set_constant_K_integrand(const mgic_ref_params *q, mgic_ref_fab *integrand,
                                       mgic_ref_fab *multigrid_vars, double dx) {
  Level out(integrand), mv(multigrid_vars);
  set_constant_K_integrand(out.data, mv.data, RealVect(dx, dx, dx), params_of(q));
}

void mgic_ref_set_regrid_condition(const mgic_ref_params *q, mgic_ref_fab *condition,
                                   mgic_ref_fab *multigrid_vars, double dx) {
  Level out(condition), mv(multigrid_vars);
  set_regrid_condition(out.data, mv.data, RealVect(dx, dx, dx), params_of(q));
}

void mgic_ref_set_update_psi0(mgic_ref_fab *multigrid_vars, mgic_ref_fab *dpsi) {
  Level mv(multigrid_vars), dp(dpsi);
  set_update_psi0(mv.data, dp.data, Copier());
}

void mgic_ref_set_output_data(const mgic_ref_params *q, mgic_ref_fab *grchombo_vars,
                              mgic_ref_fab *multigrid_vars, double dx, double constant_K) {
  Level out(grchombo_vars), mv(multigrid_vars);
  set_output_data(out.data, mv.data, params_of(q), RealVect(dx, dx, dx), constant_K);
}

double mgic_ref_set_m_value(const mgic_ref_params *q, double phi_here, double constant_K) {
  Real m = 0.0;
  set_m_value(m, phi_here, params_of(q), constant_K);
  return m;
}

double mgic_ref_get_Aij(const mgic_ref_params *q, int i, int j, double rbh1, double rbh2,
                        const double *n1, const double *n2, const double *J1, const double *J2,
                        const double *P1, const double *P2) {
  return get_Aij(i, j, rbh1, rbh2, vec(n1), vec(n2), vec(J1), vec(J2), vec(P1), vec(P2),
                 params_of(q));
}

void mgic_ref_set_binary_bh_Aij(const mgic_ref_params *q, mgic_ref_fab *multigrid_vars,
                                const int *iv, const double *loc) {
  Level mv(multigrid_vars);
  set_binary_bh_Aij(mv.fab, IntVect(iv[0], iv[1], iv[2]), vec(loc), params_of(q));
}

double mgic_ref_set_binary_bh_psi(const mgic_ref_params *q, const double *loc) {
  return set_binary_bh_psi(vec(loc), params_of(q));
}

double mgic_ref_my_phi_function(const double *loc, double amplitude, double wavelength,
                                const double *L) {
  return my_phi_function(vec(loc), amplitude, wavelength, vec(L));
}

int mgic_ref_num_multigrid_vars(void) { return NUM_MULTIGRID_VARS; }
int mgic_ref_num_grchombo_vars(void) { return NUM_GRCHOMBO_VARS; }

} /* extern "C" */
