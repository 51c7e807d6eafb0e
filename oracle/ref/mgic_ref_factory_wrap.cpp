/*
 * mgic_ref_factory_wrap.cpp -- a plain C face for the reference's operator
 * factory, set_tag_cells, set_domains_and_dx and getPoissonParameters,
 * compiled from the reference's own
 * Source/VariableCoeffPoissonOperatorFactory.cpp, Source/SetGrids.cpp and
 * Source/PoissonParameters.cpp.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/reference.py binds it).  This file is
 * this project's code: it builds levels of boxes (chombo_operator_standin.H),
 * hands them to the reference's functions and copies out what they made.  It
 * restates none of their logic.  An operator the factory returns is wrapped
 * in the handle of mgic_ref_op_wrap.cpp, whose entry points then drive it.
 *
 * MayDay::Error / MayDay::Abort inside an entry point of this file end the
 * call: the message is kept for mgic_ref_last_error() and the entry point
 * reports failure.  Outside them they are counted, as before.
 */
#include "mgic_ref_op_handle.H"

#include "PoissonParameters.H"
#include "SetGrids.H"
#include "VariableCoeffPoissonOperatorFactory.H"

#include <map>

namespace {

typedef mgic_ref_field Field;

struct mayday_thrown {};

bool g_armed = false;
std::string g_error;
std::map<std::string, std::vector<std::string>> g_deck;

/* runs f with MayDay armed; false when it called MayDay */
template <class F> bool guarded(F f) {
  g_error.clear();
  g_armed = true;
  bool ok = true;
  try {
    f();
  } catch (const mayday_thrown &) {
    ok = false;
  }
  g_armed = false;
  return ok;
}

Box box6(const int *b) { return Box(IntVect(b[0], b[1], b[2]), IntVect(b[3], b[4], b[5])); }

void put_box(const Box &b, int *out) {
  for (int d = 0; d < 3; ++d) {
    out[d] = b.smallEnd()[d];
    out[3 + d] = b.bigEnd()[d];
  }
}

[[noreturn]] void no_grid_generation() {
  MayDay::Abort("grid generation is not part of the stand-in");
  throw mayday_thrown();
}

} // namespace

void mgic_ref_mayday_raise(const char *message) {
  if (!g_armed) {
    mgic_ref_mayday();
    return;
  }
  g_error = message ? message : "";
  throw mayday_thrown();
}

/* what set_grids names and nothing calls */
BRMeshRefine::BRMeshRefine(const ProblemDomain &, const Vector<int> &, Real, int, int, int) { no_grid_generation(); }
int BRMeshRefine::regrid(Vector<Vector<Box>> &, Vector<IntVectSet> &, int, int, const Vector<Vector<Box>> &) {
  no_grid_generation();
}
void domainSplit(const ProblemDomain &, Vector<Box> &, int, int) { no_grid_generation(); }
int LoadBalance(Vector<int> &, const Vector<Box> &) { no_grid_generation(); }
void set_initial_conditions(LevelData<FArrayBox> &, LevelData<FArrayBox> &, const RealVect &,
                            const PoissonParameters &) {
  no_grid_generation();
}
void set_regrid_condition(LevelData<FArrayBox> &, LevelData<FArrayBox> &, const RealVect &,
                          const PoissonParameters &) {
  no_grid_generation();
}

extern "C" {

const char *mgic_ref_last_error(void) { return g_error.c_str(); }

/* ---- the deck ParmParse reads ---- */
void mgic_ref_deck_clear(void) { g_deck.clear(); }
void mgic_ref_deck_add(const char *name, const char *word) { g_deck[name].push_back(word); }
int mgic_ref_deck_count(const char *name) {
  const auto it = g_deck.find(name);
  return it == g_deck.end() ? -1 : (int)it->second.size();
}
const char *mgic_ref_deck_word(const char *name, int n) { return g_deck[name][n].c_str(); }

/* ---- getPoissonParameters: every field of the class ---- */
struct mgic_ref_poisson_parameters {
  int nCells[3], maxGridSize, blockFactor, bufferSize;
  double fillRatio, refineThresh;
  int coefficient_average_type, verbosity, maxLevel, numLevels;
  int n_periodic, periodic[8], n_refRatio, refRatio[32];
  int domain[6], domain_periodic[3];
  double coarsestDx, domainLength[3], probLo[3], probHi[3], alpha, beta, G_Newton, phi_amplitude,
      phi_wavelength, bh1_bare_mass, bh2_bare_mass, bh1_spin, bh2_spin, bh1_momentum, bh2_momentum,
      bh1_offset, bh2_offset;
};

int mgic_ref_get_poisson_parameters(mgic_ref_poisson_parameters *out) {
  PoissonParameters p{};
  if (!guarded([&] { getPoissonParameters(p); })) return 1;
  std::memset(out, 0, sizeof *out);
  for (int d = 0; d < 3; ++d) {
    out->nCells[d] = p.nCells[d];
    out->domainLength[d] = p.domainLength[d];
    out->probLo[d] = p.probLo[d];
    out->probHi[d] = p.probHi[d];
    out->domain_periodic[d] = p.coarsestDomain.isPeriodic(d);
  }
  put_box(p.coarsestDomain.domainBox(), out->domain);
  out->maxGridSize = p.maxGridSize;
  out->blockFactor = p.blockFactor;
  out->bufferSize = p.bufferSize;
  out->fillRatio = p.fillRatio;
  out->refineThresh = p.refineThresh;
  out->coefficient_average_type = p.coefficient_average_type;
  out->verbosity = p.verbosity;
  out->maxLevel = p.maxLevel;
  out->numLevels = p.numLevels;
  out->n_periodic = (int)p.periodic.size();
  for (int n = 0; n < out->n_periodic && n < 8; ++n) out->periodic[n] = p.periodic[n];
  out->n_refRatio = (int)p.refRatio.size();
  for (int n = 0; n < out->n_refRatio && n < 32; ++n) out->refRatio[n] = p.refRatio[n];
  out->coarsestDx = p.coarsestDx;
  out->alpha = p.alpha;
  out->beta = p.beta;
  out->G_Newton = p.G_Newton;
  out->phi_amplitude = p.phi_amplitude;
  out->phi_wavelength = p.phi_wavelength;
  out->bh1_bare_mass = p.bh1_bare_mass;
  out->bh2_bare_mass = p.bh2_bare_mass;
  out->bh1_spin = p.bh1_spin;
  out->bh2_spin = p.bh2_spin;
  out->bh1_momentum = p.bh1_momentum;
  out->bh2_momentum = p.bh2_momentum;
  out->bh1_offset = p.bh1_offset;
  out->bh2_offset = p.bh2_offset;
  return 0;
}

/* ---- set_domains_and_dx: domains nlevels * 6, dx nlevels ---- */
int mgic_ref_set_domains_and_dx(int nlevels, const int *domain0, const int *periodic, double dx0,
                                const int *ref_ratio, int *domains, int *periodic_out, double *dx) {
  PoissonParameters p{};
  const bool per[3] = {periodic[0] != 0, periodic[1] != 0, periodic[2] != 0};
  p.numLevels = nlevels;
  p.coarsestDx = dx0;
  p.coarsestDomain = ProblemDomain(box6(domain0), per);
  p.refRatio = Vector<int>(ref_ratio, ref_ratio + nlevels);
  Vector<ProblemDomain> vd;
  Vector<Real> vdx;
  if (!guarded([&] { set_domains_and_dx(vd, vdx, p); })) return 1;
  if ((int)vd.size() != nlevels || (int)vdx.size() != nlevels) return 2;
  for (int l = 0; l < nlevels; ++l) {
    put_box(vd[l].domainBox(), domains + 6 * l);
    for (int d = 0; d < 3; ++d) periodic_out[3 * l + d] = vd[l].isPeriodic(d);
    dx[l] = vdx[l];
  }
  return 0;
}

/* ---- set_tag_cells ----
 * levels of boxes (nbox[l] boxes each, all concatenated in `boxes`) with one
 * value per valid cell (concatenated box after box in `values`), the domain
 * of every level; returns a handle that holds the tags */
struct mgic_ref_tags {
  Vector<IntVectSet> tags;
};

mgic_ref_tags *mgic_ref_set_tag_cells(int nlevels, const int *nbox, const int *boxes, const int *domains,
                                      const int *periodic, const double *values, const double *dx,
                                      double refine_thresh, int tags_grow, int base_level) {
  const bool per[3] = {periodic[0] != 0, periodic[1] != 0, periodic[2] != 0};
  Vector<ProblemDomain> vd;
  Vector<Real> vdx(dx, dx + nlevels);
  std::vector<std::unique_ptr<Field>> own;
  Vector<Field *> rhs;
  for (int l = 0; l < nlevels; ++l) {
    vd.push_back(ProblemDomain(box6(domains + 6 * l), per));
    Vector<Box> bs;
    for (int n = 0; n < nbox[l]; ++n, boxes += 6) bs.push_back(box6(boxes));
    own.emplace_back(new Field(DisjointBoxLayout(bs, vd[l]), 1, IntVect::Zero));
    rhs.push_back(own.back().get());
    for (DataIterator dit = rhs[l]->dataIterator(); dit.ok(); ++dit) {
      FArrayBox &fab = (*rhs[l])[dit];
      std::memcpy(fab.dataPtr(), values, sizeof(double) * (size_t)fab.box().numPts());
      values += fab.box().numPts();
    }
  }
  mgic_ref_tags *t = new mgic_ref_tags;
  t->tags.resize(nlevels);
  if (!guarded([&] { set_tag_cells(rhs, t->tags, vdx, vd, refine_thresh, tags_grow, base_level, nlevels); })) {
    delete t;
    return nullptr;
  }
  return t;
}

long mgic_ref_tags_count(const mgic_ref_tags *t, int level) { return t->tags[level].numPts(); }

/* (i, j, k) of every tagged cell of a level, ordered by k, then j, then i */
void mgic_ref_tags_get(const mgic_ref_tags *t, int level, int *ijk) {
  for (const std::array<int, 3> &c : t->tags[level].cells()) {
    *ijk++ = c[2];
    *ijk++ = c[1];
    *ijk++ = c[0];
  }
}

void mgic_ref_tags_destroy(mgic_ref_tags *t) { delete t; }

/* ---- the factory ---- */
struct mgic_ref_factory {
  std::unique_ptr<AMRLevelOpFactory<Field>> fac;
  Vector<DisjointBoxLayout> grids;
  Vector<ProblemDomain> domains;
  Vector<RefCountedPtr<Field>> a, b;
  mgic_ref_parm parm;
};

/* by_deck 0: VariableCoeffPoissonOperatorFactory::define with m_coefficient_average_type as the
 * constructor left it (average_type < 0) or set to average_type; by_deck 1: defineOperatorFactory
 * with a PoissonParameters whose coefficient_average_type is average_type.  The coefficients are
 * created with coef_ghost layers and left unwritten. */
mgic_ref_factory *mgic_ref_factory_create(int nlevels, const int *nbox, const int *boxes, const int *domain0,
                                          const int *periodic, const int *ref_ratio, double dx0, double alpha,
                                          double beta, const int *bc_lo, const int *bc_hi, double bc_value,
                                          int coef_ghost, int by_deck, int average_type) {
  mgic_ref_factory *f = new mgic_ref_factory;
  const bool per[3] = {periodic[0] != 0, periodic[1] != 0, periodic[2] != 0};
  const Vector<int> ratios(ref_ratio, ref_ratio + nlevels);
  for (int l = 0; l < nlevels; ++l) {
    f->domains.push_back(l == 0 ? ProblemDomain(box6(domain0), per) : refine(f->domains[l - 1], ratios[l - 1]));
    Vector<Box> bs;
    for (int n = 0; n < nbox[l]; ++n, boxes += 6) bs.push_back(box6(boxes));
    f->grids.push_back(DisjointBoxLayout(bs, f->domains[l]));
    const IntVect g(coef_ghost, coef_ghost, coef_ghost);
    f->a.push_back(RefCountedPtr<Field>(new Field(f->grids[l], 1, g)));
    f->b.push_back(RefCountedPtr<Field>(new Field(f->grids[l], 1, g)));
  }
  for (int d = 0; d < 3; ++d) {
    f->parm.bc_lo[d] = bc_lo[d];
    f->parm.bc_hi[d] = bc_hi[d];
  }
  f->parm.bc_value = bc_value;
  const bool ok = guarded([&] {
    if (by_deck) {
      PoissonParameters p{};
      p.coarsestDomain = f->domains[0];
      p.refRatio = ratios;
      p.coarsestDx = dx0;
      p.alpha = alpha;
      p.beta = beta;
      p.numLevels = nlevels;
      p.coefficient_average_type = average_type;
      f->fac.reset(defineOperatorFactory(f->grids, f->domains, f->a, f->b, p));
    } else {
      VariableCoeffPoissonOperatorFactory *made = new VariableCoeffPoissonOperatorFactory;
      f->fac.reset(made);
      made->define(f->domains[0], f->grids, ratios, dx0, BCHolder(ParseBC), alpha, f->a, beta, f->b);
      if (average_type >= 0) made->m_coefficient_average_type = average_type;
    }
  });
  if (!ok) {
    delete f;
    return nullptr;
  }
  return f;
}

void mgic_ref_factory_destroy(mgic_ref_factory *f) { delete f; }

int mgic_ref_factory_average_type(const mgic_ref_factory *f) {
  return static_cast<const VariableCoeffPoissonOperatorFactory *>(f->fac.get())->m_coefficient_average_type;
}

/* which: 0 aCoef, 1 bCoef; the whole fab, ghosts included */
void mgic_ref_factory_coef_set(mgic_ref_factory *f, int level, int which, int box, const double *src) {
  FArrayBox &fab = (*(which ? f->b : f->a)[level])[DataIndex{box}];
  std::memcpy(fab.dataPtr(), src, sizeof(double) * (size_t)fab.box().numPts());
}

void mgic_ref_factory_coef_get(mgic_ref_factory *f, int level, int which, int box, double *dst) {
  const FArrayBox &fab = (*(which ? f->b : f->a)[level])[DataIndex{box}];
  std::memcpy(dst, fab.dataPtr(), sizeof(double) * (size_t)fab.box().numPts());
}

} /* extern "C" */

namespace {

/* the handle mgic_ref_op_* drive, around an operator the factory made */
mgic_ref_op *wrap(mgic_ref_factory *f, VariableCoeffPoissonOperator *made) {
  mgic_ref_op *o = new mgic_ref_op;
  o->op = static_cast<mgic_ref_op_class *>(made);
  o->parm = f->parm;
  o->fine = made->m_aCoef->disjointBoxLayout();
  coarsen_dbl(o->coarse, o->fine, 2);
  return o;
}

} // namespace

extern "C" {

/* status: 0 an operator, 1 the factory returned NULL, 2 it called MayDay */
mgic_ref_op *mgic_ref_factory_mg_new_op(mgic_ref_factory *f, int level, int depth, int *status) {
  MGLevelOp<Field> *made = nullptr;
  if (!guarded([&] { made = f->fac->MGnewOp(f->domains[level], depth, true); })) {
    *status = 2;
    return nullptr;
  }
  *status = made ? 0 : 1;
  return made ? wrap(f, dynamic_cast<VariableCoeffPoissonOperator *>(made)) : nullptr;
}

mgic_ref_op *mgic_ref_factory_amr_new_op(mgic_ref_factory *f, const int *domain, int *status) {
  AMRLevelOp<Field> *made = nullptr;
  const bool per[3] = {false, false, false};
  if (!guarded([&] { made = f->fac->AMRnewOp(ProblemDomain(box6(domain), per)); })) {
    *status = 2;
    return nullptr;
  }
  *status = 0;
  return wrap(f, dynamic_cast<VariableCoeffPoissonOperator *>(made));
}

int mgic_ref_factory_ref_to_finer(mgic_ref_factory *f, const int *domain, int *ratio) {
  const bool per[3] = {false, false, false};
  return guarded([&] { *ratio = f->fac->refToFiner(ProblemDomain(box6(domain), per)); }) ? 0 : 2;
}

/* ---- what a made operator holds ---- */
void mgic_ref_op_info(const mgic_ref_op *o, double *dx_dxcrse_alpha_beta, int *ref_coarser_finer, int *nbox,
                      int *coef_ghost, int *domain, int *periodic) {
  dx_dxcrse_alpha_beta[0] = o->op->m_dx;
  dx_dxcrse_alpha_beta[1] = o->op->m_dxCrse;
  dx_dxcrse_alpha_beta[2] = o->op->m_alpha;
  dx_dxcrse_alpha_beta[3] = o->op->m_beta;
  ref_coarser_finer[0] = o->op->m_refToCoarser;
  ref_coarser_finer[1] = o->op->m_refToFiner;
  *nbox = o->fine.size();
  coef_ghost[0] = o->op->m_aCoef->ghostVect()[0];
  coef_ghost[1] = o->op->m_bCoef->ghostVect()[0];
  put_box(o->op->m_domain.domainBox(), domain);
  for (int d = 0; d < 3; ++d) periodic[d] = o->op->m_domain.isPeriodic(d);
}

void mgic_ref_op_box(const mgic_ref_op *o, int box, int *lohi) { put_box(o->fine[DataIndex{box}], lohi); }

/* which: 0 m_aCoef, 1 m_bCoef; the whole fab, ghosts included */
void mgic_ref_op_coef_get(const mgic_ref_op *o, int which, int box, double *dst) {
  const FArrayBox &fab = (*(which ? o->op->m_bCoef : o->op->m_aCoef))[DataIndex{box}];
  std::memcpy(dst, fab.dataPtr(), sizeof(double) * (size_t)fab.box().numPts());
}

/* the cells the operator's exchange copier fills, as (to box, lo, hi, from box, shift): 11 ints each */
int mgic_ref_op_copier_count(const mgic_ref_op *o) { return (int)o->op->m_exchangeCopier.motions().size(); }
void mgic_ref_op_copier_get(const mgic_ref_op *o, int *out) {
  for (const Copier::Item &m : o->op->m_exchangeCopier.motions()) {
    *out++ = m.to;
    put_box(m.cells, out);
    out += 6;
    *out++ = m.from;
    for (int d = 0; d < 3; ++d) *out++ = m.shift[d];
  }
}

} /* extern "C" */
