"""Cases, inputs and runners shared by tests/test_reference_operator.py and
tests/golden/make_golden.py (reference_operator.npz).  Test infrastructure only.

A case is one level of boxes over a domain with a boundary table and
coefficients; an operation is one call of the operator class on fresh inputs.
Each (case, operation) is run three ways on the SAME inputs: by the reference's
own VariableCoeffPoissonOperator.cpp / SetBCs.cpp, compiled
(oracle.reference.Operator), by the oracle's restatement (oracle.OracleMG) and
by the HIP entry points mgic_op_* (run_device).  Every runner returns
{name: [one array per box]} of the fields the call may write.
"""
import collections
import os

import numpy as np

import oracle
from oracle import reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_operator.npz")

Case = collections.namedtuple(
    "Case", "name domain boxes periodic bc_lo bc_hi bc_value alpha beta bvar asign dx ops "
            "ghost_zero special fused fixture")

AB1, AB2 = (1.0, -1.0), (0.75, -1.3)
# lambda's shift is 2 * 3 * beta / (dx * dx), evaluated left to right.  The
# pairs (beta, dx) the cases use are ones at which the other ways of grouping
# it round to another double: at (-1.3, 0.7) all of 2 * 3 * (beta / (dx * dx)),
# 2 * 3 * beta / dx / dx and (2 * 3 * beta) * (1 / (dx * dx)); at (-1, 0.7) the
# first and the third, at (-1, 0.37) the second (GROUPINGS, checked on import).
DX1, DX2 = 0.37, 0.7
GROUPINGS = (lambda b, h: 2.0 * 3 * (b / (h * h)), lambda b, h: 2.0 * 3 * b / h / h,
             lambda b, h: (2.0 * 3 * b) * (1.0 / (h * h)))
for _b, _h, _which in ((-1.3, DX2, (0, 1, 2)), (-1.0, DX2, (0, 2)), (-1.0, DX1, (1,))):
    assert all(GROUPINGS[_n](_b, _h) != 2.0 * 3 * _b / (_h * _h) for _n in _which)

# boundary tables: (bc_lo, bc_hi, bc_value)
DIRI0 = ((0, 0, 0), (0, 0, 0), 0.0)
DIRI = ((0, 0, 0), (0, 0, 0), 0.25)       # inhomogeneous Dirichlet
NEUM = ((1, 1, 1), (1, 1, 1), 0.25)
# no face has the rule of the face opposite or of both its neighbours' lows
SIX = ((0, 1, 0), (1, 0, 1), 0.25)

RELAX = ("relax1", "relax2", "relax3", "relax4")
ALL_OPS = ("res_inhom", "res_hom", "op_inhom", "op_hom", "op_nobc", "precond") + RELAX + (
    "gsrb", "jacobi", "restrict", "lambda", "bc_inhom", "bc_hom")
NO_RESTRICT = tuple(o for o in ALL_OPS if o != "restrict")
BIG_OPS = ("relax2", "relax4", "precond", "restrict")


def _dom(n):
    return (0, 0, 0, n[0] - 1, n[1] - 1, n[2] - 1)


def _cut(n, parts):
    """The domain of extents n cut into parts[d] equal pieces along d."""
    out = []
    for kz in range(parts[2]):
        for jy in range(parts[1]):
            for ix in range(parts[0]):
                p = (ix, jy, kz)
                lo = [p[d] * (n[d] // parts[d]) for d in range(3)]
                hi = [lo[d] + n[d] // parts[d] - 1 for d in range(3)]
                out.append(tuple(lo + hi))
    return out


def _case(name, n, parts, bc, ab, bvar, asign, dx, ops=ALL_OPS, periodic=(0, 0, 0), ghost_zero=False,
          special=False, fused=1, fixture=True):
    return Case(name, _dom(n), _cut(n, parts), periodic, bc[0], bc[1], bc[2], ab[0], ab[1], bvar,
                asign, dx, ops, ghost_zero, special, fused, fixture)


ONE = (1, 1, 1)
CASES = [
    _case("1box-diri0", (8, 6, 4), ONE, DIRI0, AB1, False, -1, DX1),
    _case("1box-diri-bvar-aboth", (8, 6, 4), ONE, DIRI, AB2, True, 0, DX2),
    _case("1box-neum-bvar", (8, 6, 4), ONE, NEUM, AB1, True, -1, DX2),
    _case("1box-six-apos", (8, 6, 4), ONE, SIX, AB2, False, +1, DX2),
    _case("ragged-six-bvar", (13, 7, 5), ONE, SIX, AB1, True, 0, DX1, ops=NO_RESTRICT),
    _case("ragged-diri", (13, 7, 5), ONE, DIRI, AB2, False, -1, DX2, ops=NO_RESTRICT),
    # flag 2 on the periodic direction: ParseBC never looks at it there
    _case("2box-periodic-x-flag2", (16, 16, 8), (2, 1, 1), ((2, 1, 0), (2, 0, 1), 0.25), AB1, True, -1,
          DX1, periodic=(1, 0, 0)),
    _case("4box-periodic-y-diri", (16, 16, 8), (2, 2, 1), DIRI, AB2, False, 0, DX2, periodic=(0, 1, 0)),
    # flag 2 on a side that is NOT periodic: the reference leaves that ghost
    # as it was; the inputs' ghosts hold zero there (the device keeps no other)
    _case("1box-flag2-nonperiodic", (8, 6, 4), ONE, ((2, 0, 1), (0, 2, 0), 0.25), AB1, True, -1, DX1,
          ghost_zero=True),
    # rhs = the reference's own applyOpI(dpsi, homogeneous): restriction, which
    # forms the operator by the same expression, meets a residual that is
    # exactly zero ("zres_restrict" takes rhs from "op_hom"'s result)
    _case("1box-zero-residual", (8, 6, 4), ONE, DIRI, AB2, True, -1, DX2,
          ops=("op_hom", "zres_restrict")),
    _case("special-values", (12, 10, 6), ONE, SIX, AB2, True, -1, DX2,
          ops=("res_inhom", "res_hom", "op_inhom", "op_hom", "op_nobc"), special=True),
    # the smallest shapes that reach the kernels the small boxes do not (too
    # large for the fixture): 3 x 3 two-sweep tiles of 64 x 22, one interior,
    # ragged last tiles (constant b, streaming forced), and the 132 x 17
    # streaming tile (129..132 wide, cell-varying b)
    _case("136x52x12-six", (136, 52, 12), ONE, SIX, AB1, False, -1, DX1, ops=BIG_OPS, fused=2,
          fixture=False),
    _case("136x52x12-diri", (136, 52, 12), ONE, DIRI, AB2, False, -1, DX2, ops=BIG_OPS, fused=2,
          fixture=False),
    _case("130x20x6-six", (130, 20, 6), ONE, SIX, AB2, True, -1, DX2, ops=BIG_OPS, fused=2,
          fixture=False),
    _case("130x20x6-diri", (130, 20, 6), ONE, DIRI, AB1, True, -1, DX1, ops=BIG_OPS, fused=2,
          fixture=False),
]
CASE = {c.name: c for c in CASES}
PAIRS = [(c.name, op) for c in CASES for op in c.ops]
# a bogus flag: the reference calls MayDay::Error once per offending face
BOGUS = _case("bogus-flag", (8, 6, 4), ONE, ((0, 7, 0), (0, 0, 0), 0.25), AB1, False, -1, DX1, ops=())

SPECIALS = (-0.0, 3e-310, 1e300, np.inf, np.nan, 0.0)
SPECIAL_CENTRES = ((1, 1, 1), (5, 1, 1), (9, 1, 1), (1, 6, 3), (5, 6, 3), (9, 6, 3))


def shape(b, g=0):
    return tuple(b[3 + d] - b[d] + 1 + 2 * g for d in (2, 1, 0))


def coarse_boxes(c):
    return [tuple(v // 2 for v in b) for b in c.boxes]


def restrictable(c):
    return all(b[d] % 2 == 0 and (b[3 + d] + 1) % 2 == 0 for b in c.boxes for d in range(3))


def inner(a):
    return np.ascontiguousarray(a[1:-1, 1:-1, 1:-1])


def faces(full):
    """The six one-deep face slabs of a ghosted array (edges and corners left out)."""
    return [full[1:-1, 1:-1, 0], full[1:-1, 1:-1, -1], full[1:-1, 0, 1:-1], full[1:-1, -1, 1:-1],
            full[0, 1:-1, 1:-1], full[-1, 1:-1, 1:-1]]


def inputs(c):
    """Deterministic inputs: {name: [array per box]}.  dpsi, cor0 (what the
    preconditioner's output held) and coarse0 (what the coarse residual held)
    are ghosted and their ghosts hold values no neighbour has, so a refill
    that is skipped shows."""
    names = [x.name for x in CASES] + [BOGUS.name]
    rng = np.random.default_rng([20261021, names.index(c.name)])
    a_range = {-1: (-2.0, -0.5), +1: (0.5, 2.0), 0: (-2.0, 2.0)}[c.asign]
    d = collections.defaultdict(list)
    for b, cb in zip(c.boxes, coarse_boxes(c)):
        for k in ("dpsi", "cor0"):
            x = rng.uniform(-1, 1, shape(b, 1))
            if c.ghost_zero:
                v = inner(x)
                x = np.zeros_like(x)
                x[1:-1, 1:-1, 1:-1] = v
            d[k].append(x)
        d["rhs"].append(rng.uniform(-1, 1, shape(b)))
        d["a"].append(rng.uniform(*a_range, shape(b)))
        d["b"].append(rng.uniform(0.5, 2.0, shape(b)) if c.bvar
                      else np.full(shape(b), 1.0 if c.alpha == 1.0 else 1.7))
        d["coarse0"].append(rng.uniform(-1, 1, shape(cb, 1)))
    if c.special:
        for m, (ci, cj, ck) in enumerate(SPECIAL_CENTRES):
            d["dpsi"][0][ck:ck + 3, cj:cj + 3, ci:ci + 3] = SPECIALS[m]
            d["rhs"][0][ck, cj, ci] = SPECIALS[(m + 1) % len(SPECIALS)]
    # lambda must be finite: alpha a + 6 beta / dx^2 stays away from zero
    for a in d["a"]:
        assert np.all(np.abs(c.alpha * a + 6.0 * c.beta / (c.dx * c.dx)) > 0.5)
    return dict(d)


def _nbox(c):
    return range(len(c.boxes))


# ------------------------------------------------------------------ the compiled reference
def reference_operator(c, d):
    """(operator, fields): the reference's operator as its factory leaves it."""
    R = ref.Operator(c.boxes, c.domain, c.dx, c.alpha, c.beta, c.periodic, c.bc_lo, c.bc_hi,
                     c.bc_value)
    f = dict(a=R.field(0, values=d["a"]), b=R.field(0, values=d["b"]),
             rhs=R.field(0, values=d["rhs"]), lhs=R.field(0), dpsi=R.field(1), cor=R.field(1))
    for n in _nbox(c):
        R.set(f["dpsi"], n, d["dpsi"][n], full=True)
        R.set(f["cor"], n, d["cor0"][n], full=True)
    if restrictable(c):
        f["coarse"] = R.field(1, level=1)
        for n in _nbox(c):
            R.set(f["coarse"], n, d["coarse0"][n], full=True)
    R.set_coefs(f["a"], f["b"], c.alpha, c.beta)
    R.compute_lambda()
    return R, f


def run_reference(c, d, op, rhs=None):
    R, f = reference_operator(c, d)
    if rhs is not None:
        for n in _nbox(c):
            R.set(f["rhs"], n, rhs[n])
    get = lambda k, full=False: [R.get(f[k], n, full) for n in _nbox(c)]
    if op in ("res_inhom", "res_hom"):
        R.residual(f["lhs"], f["dpsi"], f["rhs"], op != "res_inhom")
        return dict(lhs=get("lhs"))
    if op in ("op_inhom", "op_hom"):
        R.apply_op(f["lhs"], f["dpsi"], op == "op_hom")
        return dict(lhs=get("lhs"))
    if op == "op_nobc":
        R.apply_op_no_boundary(f["lhs"], f["dpsi"])
        return dict(lhs=get("lhs"))
    if op == "precond":
        R.precond(f["cor"], f["rhs"])
        return dict(cor=get("cor"))
    if op in RELAX:
        R.relax(f["dpsi"], f["rhs"], int(op[-1]))
        return dict(dpsi=get("dpsi"))
    if op == "gsrb":
        R.level_gsrb(f["dpsi"], f["rhs"])
        return dict(dpsi=get("dpsi"))
    if op == "jacobi":
        R.level_jacobi(f["dpsi"], f["rhs"])
        return dict(dpsi=get("dpsi"))
    if op in ("restrict", "zres_restrict"):
        R.restrict_residual(f["coarse"], f["dpsi"], f["rhs"])
        return dict(coarse=get("coarse"))
    if op == "lambda":
        return {"lambda": [R.lam(n) for n in _nbox(c)]}
    if op in ("bc_inhom", "bc_hom"):
        for n in _nbox(c):
            R.parse_bc(f["dpsi"], n, op == "bc_hom")
        return dict(full=get("dpsi", True))
    raise KeyError(op)


# ------------------------------------------------------------------ the oracle
def oracle_mg(c, d, alpha=None, beta=None):
    o = oracle.OracleMG(c.boxes, c.domain, c.dx, alpha=c.alpha if alpha is None else alpha,
                        beta=c.beta if beta is None else beta, periodic=c.periodic, bc_lo=c.bc_lo,
                        bc_hi=c.bc_hi, bc_value=c.bc_value, nlevels=2 if restrictable(c) else 1)
    for n in _nbox(c):
        o.set(0, oracle.ACOEF, n, d["a"][n])
        o.set(0, oracle.BCOEF, n, d["b"][n])
        o.set(0, oracle.RHS, n, d["rhs"][n])
        o.set(0, oracle.PHI, n, d["dpsi"][n], full=True)
        o.set(0, oracle.CORR, n, d["cor0"][n], full=True)
        if restrictable(c):
            o.set(1, oracle.RESID, n, d["coarse0"][n], full=True)
    o.setup()
    return o


def run_oracle(c, d, op, rhs=None):
    o = oracle_mg(c, d)
    if rhs is not None:
        for n in _nbox(c):
            o.set(0, oracle.RHS, n, rhs[n])
    get = lambda k, lev=0, full=False: [o.get(lev, k, n, full) for n in _nbox(c)]
    if op in ("res_inhom", "res_hom"):
        o.residual(0, oracle.TMP, oracle.PHI, oracle.RHS, op != "res_inhom")
        return dict(lhs=get(oracle.TMP))
    if op in ("op_inhom", "op_hom"):
        o.apply_op(0, oracle.TMP, oracle.PHI, op == "op_hom")
        return dict(lhs=get(oracle.TMP))
    if op == "op_nobc":
        # applyOpNoBoundary: the exchange, then the kernel box by box
        o.exchange(0, oracle.PHI)
        out = []
        for n, b in enumerate(c.boxes):
            lo, hi = b[:3], b[3:]
            lof = oracle.Fab(np.zeros(shape(b)), lo)
            oracle.apply_op(lof, oracle.Fab(o.get(0, oracle.PHI, n, full=True), [v - 1 for v in lo]),
                            c.alpha, oracle.Fab(d["a"][n].copy(), lo), c.beta,
                            oracle.Fab(d["b"][n].copy(), lo), lo, hi, c.dx)
            out.append(lof.arr)
        return dict(lhs=out)
    if op == "precond":
        o.precond(0, oracle.CORR, oracle.RHS)
        return dict(cor=get(oracle.CORR))
    if op in RELAX:
        o.relax(0, oracle.PHI, oracle.RHS, int(op[-1]))
        return dict(dpsi=get(oracle.PHI))
    if op == "gsrb":
        o.level_gsrb(0, oracle.PHI, oracle.RHS)
        return dict(dpsi=get(oracle.PHI))
    if op == "jacobi":
        o.level_jacobi(0, oracle.PHI, oracle.RHS)
        return dict(dpsi=get(oracle.PHI))
    if op in ("restrict", "zres_restrict"):
        o.restrict_residual(0, oracle.PHI, oracle.RHS)
        return dict(coarse=get(oracle.RESID, 1))
    if op == "lambda":
        return {"lambda": get(oracle.LAMBDA)}
    if op in ("bc_inhom", "bc_hom"):
        o.fill_bc(0, oracle.PHI, op == "bc_hom")
        return dict(full=get(oracle.PHI, 0, True))
    raise KeyError(op)


# ------------------------------------------------------------------ the device
class Device:
    """Grid, coefficient fields, factory and operator of one case on the GPU:
    set up once per case, the data fields uploaded afresh by every run."""

    def __init__(self, mg, comm, c, d):
        self.mg, self.c = mg, c
        self.grid = mg.Grid(comm, c.domain, c.boxes, c.dx, periodic=c.periodic)
        self.f = {k: mg.LevelData(self.grid) for k in ("a", "b", "rhs", "lhs", "dpsi", "cor")}
        for n in _nbox(c):
            self.f["a"].upload(n, d["a"][n])
            self.f["b"].upload(n, d["b"][n])
        prm = mg.OperatorParams(alpha=c.alpha, beta=c.beta, bc_lo=c.bc_lo, bc_hi=c.bc_hi,
                                bc_value=c.bc_value, fused_smoother=c.fused)
        self.factory = mg.defineOperatorFactory(self.grid, self.f["a"], self.f["b"], prm)
        self.op = self.factory.AMRnewOp()
        if restrictable(c):
            self.cgrid = self.grid.coarsen(2)
            self.f["coarse"] = mg.LevelData(self.cgrid)

    def run(self, d, op, rhs=None):
        c, f, o = self.c, self.f, self.op
        f["lhs"].set_val_all(0.0)
        for n in _nbox(c):
            f["rhs"].upload(n, (rhs or d["rhs"])[n])
            f["dpsi"].upload(n, d["dpsi"][n], with_ghosts=True)
            f["cor"].upload(n, d["cor0"][n], with_ghosts=True)
            if "coarse" in f:
                f["coarse"].upload(n, d["coarse0"][n], with_ghosts=True)
        get = lambda x, full=False: [x.download(n, with_ghosts=full) for n in _nbox(c)]
        if op in ("res_inhom", "res_hom"):
            o.residualI(f["lhs"], f["dpsi"], f["rhs"], op != "res_inhom")
            return dict(lhs=get(f["lhs"]))
        if op in ("op_inhom", "op_hom"):
            o.applyOpI(f["lhs"], f["dpsi"], op == "op_hom")
            return dict(lhs=get(f["lhs"]))
        if op == "op_nobc":
            o.applyOpNoBoundary(f["lhs"], f["dpsi"])
            return dict(lhs=get(f["lhs"]))
        if op == "precond":
            o.preCond(f["cor"], f["rhs"])
            return dict(cor=get(f["cor"]))
        if op in RELAX:
            o.relax(f["dpsi"], f["rhs"], int(op[-1]))
            return dict(dpsi=get(f["dpsi"]))
        if op == "gsrb":
            o.levelGSRB(f["dpsi"], f["rhs"])
            return dict(dpsi=get(f["dpsi"]))
        if op == "jacobi":
            o.levelJacobi(f["dpsi"], f["rhs"])
            return dict(dpsi=get(f["dpsi"]))
        if op in ("restrict", "zres_restrict"):
            o.restrictResidual(f["coarse"], f["dpsi"], f["rhs"])
            return dict(coarse=get(f["coarse"]))
        if op == "lambda":
            return {"lambda": get(o.m_lambda)}
        if op in ("bc_inhom", "bc_hom"):
            o.fillBC(f["dpsi"], op == "bc_hom")
            return dict(full=get(f["dpsi"], True))
        raise KeyError(op)


# ------------------------------------------------------------------ the fixture
def fixture_key(case, op, name, n):
    return "/".join((case, op, name, str(n)))


def build_fixture():
    """reference_operator.npz's contents, from the compiled reference."""
    out = {}
    for c in CASES:
        if not c.fixture:
            continue
        d = inputs(c)
        rhs = None
        for op in c.ops:
            got = run_reference(c, d, op, rhs if op.startswith("zres") else None)
            if op == "op_hom":
                rhs = got["lhs"]
            for name, arrs in got.items():
                for n, a in enumerate(arrs):
                    out[fixture_key(c.name, op, name, n)] = a
    return out
