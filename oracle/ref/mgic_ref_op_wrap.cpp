/*
 * mgic_ref_op_wrap.cpp -- a plain C face for the reference's operator class
 * and ParseBC, compiled from the reference's own
 * Source/VariableCoeffPoissonOperator.cpp and Source/SetBCs.cpp.
 *
 * TEST INFRASTRUCTURE ONLY (oracle/reference.py binds it).  This file is
 * this project's code: it builds levels of boxes over a domain
 * (chombo_operator_standin.H), fills the members the reference's factory
 * would fill and calls the reference's member functions.  It restates none of
 * their logic.  A translation unit of its own, beside mgic_ref_wrap.cpp,
 * because that one is compiled against the one-box meaning of LevelData.
 *
 * The reference keeps the boundary flags in process-wide statics
 * (GlobalBCRS) that it parses once; every entry point here first installs
 * the calling operator's flags and value and clears s_areBCsParsed, so
 * several operators with different tables can be alive at once.  An operator
 * the reference's factory made (mgic_ref_factory_wrap.cpp) arrives in the same
 * handle and is driven by the same entry points.
 */
#include "mgic_ref_op_handle.H"

namespace {

mgic_ref_parm g_parm;

typedef mgic_ref_field Field;
typedef mgic_ref_op_class Op;

} // namespace

extern "C" {

mgic_ref_parm *mgic_ref_parm_table(void) { return &g_parm; }

} /* extern "C" */

namespace {

void activate(mgic_ref_op *o) {
  g_parm = o->parm;
  GlobalBCRS::s_areBCsParsed = false;
}

Box box6(const int *b) { return Box(IntVect(b[0], b[1], b[2]), IntVect(b[3], b[4], b[5])); }

Field &F(mgic_ref_op *o, int f) { return *o->fields[f]; }

} // namespace

extern "C" {

/* boxes: nbox * (lo0 lo1 lo2 hi0 hi1 hi2); domain the same six */
mgic_ref_op *mgic_ref_op_create(int nbox, const int *boxes, const int *domain, const int *periodic,
                                double dx, double alpha, double beta, const int *bc_lo,
                                const int *bc_hi, double bc_value) {
  mgic_ref_op *o = new mgic_ref_op;
  const bool per[3] = {periodic[0] != 0, periodic[1] != 0, periodic[2] != 0};
  const ProblemDomain pd(box6(domain), per);
  const int cdom[6] = {coarsen(IntVect(domain[0], domain[1], domain[2]), 2)[0],
                       coarsen(IntVect(domain[0], domain[1], domain[2]), 2)[1],
                       coarsen(IntVect(domain[0], domain[1], domain[2]), 2)[2],
                       coarsen(IntVect(domain[3], domain[4], domain[5]), 2)[0],
                       coarsen(IntVect(domain[3], domain[4], domain[5]), 2)[1],
                       coarsen(IntVect(domain[3], domain[4], domain[5]), 2)[2]};
  Vector<Box> fb, cb;
  for (int n = 0; n < nbox; ++n) {
    const Box b = box6(boxes + 6 * n);
    fb.push_back(b);
    cb.push_back(Box(coarsen(b.smallEnd(), 2), coarsen(b.bigEnd(), 2)));
  }
  o->fine = DisjointBoxLayout(fb, pd);
  o->coarse = DisjointBoxLayout(cb, ProblemDomain(box6(cdom), per));
  for (int d = 0; d < 3; ++d) {
    o->parm.bc_lo[d] = bc_lo[d];
    o->parm.bc_hi[d] = bc_hi[d];
  }
  o->parm.bc_value = bc_value;
  /* what the reference's factory sets on a new operator */
  o->op = new Op;
  o->op->m_exchangeCopier.exchangeDefine(o->fine, IntVect::Unit);
  o->op->m_exchangeCopier.trimEdges(o->fine, IntVect::Unit);
  o->op->m_dx = dx;
  o->op->m_dxCrse = 2.0 * dx;
  o->op->m_alpha = alpha;
  o->op->m_beta = beta;
  o->op->m_domain = pd;
  o->op->m_bc = BCHolder(ParseBC);
  return o;
}

void mgic_ref_op_destroy(mgic_ref_op *o) { delete o; }

/* a new field of one component on the fine (level 0) or coarse (1) boxes with
 * `ghost` layers, every cell zero; returns its number */
int mgic_ref_op_field(mgic_ref_op *o, int level, int ghost) {
  Field *f = new Field(level ? o->coarse : o->fine, 1, IntVect(ghost, ghost, ghost));
  for (DataIterator dit = f->dataIterator(); dit.ok(); ++dit) (*f)[dit].setVal(0.0);
  o->fields.push_back(RefCountedPtr<Field>(f));
  return (int)o->fields.size() - 1;
}

/* the whole fab of one box, ghosts included, first index fastest */
void mgic_ref_op_field_set(mgic_ref_op *o, int f, int box, const double *src) {
  FArrayBox &fab = F(o, f)[DataIndex{box}];
  std::memcpy(fab.dataPtr(), src, sizeof(double) * (size_t)fab.box().numPts());
}

void mgic_ref_op_field_get(mgic_ref_op *o, int f, int box, double *dst) {
  const FArrayBox &fab = F(o, f)[DataIndex{box}];
  std::memcpy(dst, fab.dataPtr(), sizeof(double) * (size_t)fab.box().numPts());
}

/* m_lambda's fab of one box (no ghosts); returns 0 while m_lambda is undefined */
int mgic_ref_op_lambda_get(mgic_ref_op *o, int box, double *dst) {
  if (!o->op->m_lambda.isDefined()) return 0;
  const FArrayBox &fab = o->op->m_lambda[DataIndex{box}];
  std::memcpy(dst, fab.dataPtr(), sizeof(double) * (size_t)fab.box().numPts());
  return 1;
}

void mgic_ref_op_residual(mgic_ref_op *o, int lhs, int dpsi, int rhs, int homogeneous) {
  activate(o);
  o->op->residualI(F(o, lhs), F(o, dpsi), F(o, rhs), homogeneous != 0);
}

void mgic_ref_op_apply_op(mgic_ref_op *o, int lhs, int dpsi, int homogeneous) {
  activate(o);
  o->op->applyOpI(F(o, lhs), F(o, dpsi), homogeneous != 0);
}

void mgic_ref_op_apply_op_no_boundary(mgic_ref_op *o, int lhs, int dpsi) {
  activate(o);
  o->op->applyOpNoBoundary(F(o, lhs), F(o, dpsi));
}

void mgic_ref_op_precond(mgic_ref_op *o, int cor, int res) {
  activate(o);
  o->op->preCond(F(o, cor), F(o, res));
}

void mgic_ref_op_relax(mgic_ref_op *o, int e, int r, int iterations) {
  activate(o);
  o->op->relax(F(o, e), F(o, r), iterations);
}

void mgic_ref_op_level_gsrb(mgic_ref_op *o, int dpsi, int rhs) {
  activate(o);
  o->op->levelGSRB(F(o, dpsi), F(o, rhs));
}

void mgic_ref_op_level_jacobi(mgic_ref_op *o, int dpsi, int rhs) {
  activate(o);
  o->op->levelJacobi(F(o, dpsi), F(o, rhs));
}

void mgic_ref_op_restrict_residual(mgic_ref_op *o, int res_coarse, int dpsi, int rhs) {
  activate(o);
  o->op->restrictResidual(F(o, res_coarse), F(o, dpsi), F(o, rhs));
}

void mgic_ref_op_set_alpha_beta(mgic_ref_op *o, double alpha, double beta) {
  o->op->setAlphaAndBeta(alpha, beta);
}

void mgic_ref_op_set_coefs(mgic_ref_op *o, int a, int b, double alpha, double beta) {
  o->op->setCoefs(o->fields[a], o->fields[b], alpha, beta);
}

void mgic_ref_op_reset_lambda(mgic_ref_op *o) { o->op->resetLambda(); }
void mgic_ref_op_compute_lambda(mgic_ref_op *o) { o->op->computeLambda(); }
void mgic_ref_op_set_time(mgic_ref_op *o, double t) { o->op->setTime(t); }

/* ParseBC alone on one box's fab of a field */
void mgic_ref_parse_bc(mgic_ref_op *o, int f, int box, int homogeneous) {
  activate(o);
  Field &u = F(o, f);
  ParseBC(u[DataIndex{box}], u.disjointBoxLayout()[DataIndex{box}], o->op->m_domain, o->op->m_dx,
          homogeneous != 0);
}

} /* extern "C" */
