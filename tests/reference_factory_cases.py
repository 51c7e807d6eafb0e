"""Cases, inputs and runners shared by tests/test_reference_factory.py and
tests/golden/make_golden.py (reference_factory.npz).  Test infrastructure only.

Three tables, each run by the reference's own text, compiled
(oracle.reference.Factory / tag_cells / domains_and_dx / poisson_parameters),
and by what restates it here: the oracle's multigrid setup (oracle.OracleMG),
tests/regrid_ref.py's tagging, mg_ic_code_amd.params.read_params, and on the
GPU mgic_factory_mg_new_op, AMRMultiGrid's level operators and
mgic_field_tag_lattice.

Every runner returns a flat {key: array}; keys are "<case>/<what>/...".

The fixture holds outputs only, and two things keep it small.  An array of
more than DIGEST_ABOVE values is held as the SHA-256 of its bytes (NaNs made
one NaN first, as the bitwise comparison treats them): equal digests are equal
bits.  And a case's inputs do not depend on the mode, so what "deck-absent"
gives is what "arithmetic" gives -- a CPU test holds the library to that --
and the fixture holds it once.
"""
import collections
import hashlib
import os

import numpy as np

import oracle
from oracle import amr
from oracle import reference as ref
from tests import regrid_ref

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_factory.npz")
PARAMS_TXT = os.path.join(HERE, "golden", "params.txt")

DIRI = ((0, 0, 0), (0, 0, 0), 0.25)
SIX = ((0, 1, 0), (1, 0, 1), 0.25)
ALPHA, BETA, DX = 0.75, -1.3, 0.7  # reference_operator_cases: every regrouping of lambda's shift shows

# how the factory is made and which average it ends up with: all through
# defineOperatorFactory (the `>= 0` rule, Factory.cpp:44-46); -1 keeps the
# constructor's arithmetic
MODES = collections.OrderedDict((("arithmetic", 0), ("harmonic", 1), ("deck-absent", -1)))


def restated_average(deck_value):
    """mg_ic_code_amd/nl.py's reading of the rule: a deck that names no
    average leaves the factory's arithmetic."""
    return deck_value if deck_value >= 0 else 0


FCase = collections.namedtuple("FCase", "name boxes domain periodic bc depths special")


def _fcase(name, boxes, domain=None, periodic=(0, 0, 0), bc=DIRI, depths=None, special=False):
    domain = domain or (tuple(min(b[d] for b in boxes) for d in range(3)) +
                        tuple(max(b[3 + d] for b in boxes) for d in range(3)))
    return FCase(name, [tuple(b) for b in boxes], tuple(domain), periodic, bc, depths, special)


TWO = [(0, 0, 0, 7, 15, 15), (8, 0, 0, 31, 15, 15)]
# depths: how many operators MGnewOp returns before its first NULL, worked out
# by hand from coarsenable(2^depth * 2) -- asserted against the library
SHAPES = [
    _fcase("16x8x8", [(0, 0, 0, 15, 7, 7)], bc=SIX, depths=3),
    _fcase("16x8x24-negative", [(-16, 8, -24, -1, 15, -1)], bc=SIX, depths=3),
    _fcase("8+24-diri", TWO, depths=3),        # x = 8 is no multiple of 16: the 8-wide box decides
    _fcase("8+24-periodic", TWO, periodic=(1, 1, 1), depths=3),
    _fcase("12-wide", [(0, 0, 0, 11, 11, 11)], depths=2),      # 12 % 8: NULL at depth 2
    _fcase("6-wide", [(0, 0, 0, 5, 5, 5)], depths=1),          # 6 % 4: depth 0 only
    _fcase("8-wide-at-4", [(4, 4, 4, 11, 11, 11)], depths=2),  # 8 cells allow depth 2, lo = 4 does not
]
SPECIAL = _fcase("special-values", [(0, 0, 0, 15, 7, 7)], bc=SIX, depths=3, special=True)
FCASES = SHAPES + [SPECIAL]
FCASE = {c.name: c for c in FCASES}
FPAIRS = [(c.name, m) for c in FCASES for m in MODES]

# two AMR levels: a 16^3 base and a 16^3 patch at ratio 2 away from the origin
TWO_LEVEL = dict(name="two-level", domain0=(0, 0, 0, 15, 15, 15), base=(0, 0, 0, 15, 15, 15),
                 patch=(8, 8, 16, 23, 23, 31), depths=3)  # lo = 8 is no multiple of 16

SPECIALS = (-0.0, 3e-310, 1e300, np.inf, np.nan, 0.0)
# fine cells of a 16x8x8 box, each in a depth-2 parent of its own: (i, j, k)
SPECIAL_CELLS = ((1, 1, 1), (5, 2, 1), (9, 1, 2), (13, 3, 3), (2, 5, 5), (6, 6, 6))


def shape(b, g=0):
    return tuple(b[3 + d] - b[d] + 1 + 2 * g for d in (2, 1, 0))


def coarsen(b, r):
    return tuple(v // r for v in b)


def _seed(name, extra=0):
    names = [c.name for c in FCASES] + [TWO_LEVEL["name"]]
    return [20261021, 7, names.index(name), extra]


DIGEST_ABOVE = 1024


def digest(a):
    """SHA-256 of an array's shape and bits, every NaN made the same NaN."""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    h = hashlib.sha256(repr(a.shape).encode() + np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def is_digest(a):
    return a.dtype == np.uint8


def pairwise(x, harmonic):
    """Ratio 2 twice (the misreading): average a (nz, ny, nx) array by 2, once."""
    s = np.zeros(tuple(v // 2 for v in x.shape))
    for kk in range(2):
        for jj in range(2):
            for ii in range(2):
                v = x[kk::2, jj::2, ii::2]
                s = s + (1.0 / v if harmonic else v)
    return 1.0 / (s * 0.125) if harmonic else s * 0.125


def direct4(x, harmonic):
    s = np.zeros(tuple(v // 4 for v in x.shape))
    for kk in range(4):
        for jj in range(4):
            for ii in range(4):
                v = x[kk::4, jj::4, ii::4]
                s = s + (1.0 / v if harmonic else v)
    return 1.0 / (s * (1.0 / 64)) if harmonic else s * (1.0 / 64)


def finputs(c, mode):
    """{a, b: [per box], phi[d], rhs[d]: [per box] for each depth d}.  phi is
    ghosted and its ghosts hold values no neighbour has."""
    with np.errstate(all="ignore"):
        extra = 0
        while True:  # another seed if the inputs could not tell the misreadings apart
            rng = np.random.default_rng(_seed(c.name, extra))
            d = dict(a=[rng.uniform(-2.0, -0.5, shape(b)) for b in c.boxes],
                     b=[rng.uniform(0.5, 2.0, shape(b)) for b in c.boxes])
            for n in range(c.depths):
                r = 1 << n
                d[f"phi{n}"] = [rng.uniform(-1, 1, shape(coarsen(b, r), 1)) for b in c.boxes]
                d[f"rhs{n}"] = [rng.uniform(-1, 1, shape(coarsen(b, r))) for b in c.boxes]
            if c.special:
                harm = MODES[mode] == 1
                for m, (i, j, k) in enumerate(SPECIAL_CELLS):
                    if SPECIALS[m] == 0.0 and m == 5 and not harm:
                        continue  # the exact zero is harmonic's case (1 / 0)
                    d["a"][0][k, j, i] = SPECIALS[m]
                    d["b"][0][k, j, i] = SPECIALS[(m + 2) % 5]
            if c.depths < 3 or c.special or distinguishes(d):
                return d
            extra += 1


def distinguishes(d):
    """Pairwise ratio-2 averaging twice differs bitwise from the direct ratio
    4, and arithmetic differs from harmonic, for every coefficient array."""
    for k in ("a", "b"):
        for x in d[k]:
            for h in (0, 1):
                if np.array_equal(pairwise(pairwise(x, h), h), direct4(x, h)):
                    return False
            if np.array_equal(direct4(x, 0), direct4(x, 1)) or np.array_equal(pairwise(x, 0), pairwise(x, 1)):
                return False
    return True


# ------------------------------------------------------------------ the compiled reference
def reference_factory(c, d, mode, **kw):
    return ref.Factory([c.boxes], c.domain, DX, [d["a"]], [d["b"]], alpha=ALPHA, beta=BETA,
                       periodic=c.periodic, bc_lo=c.bc[0], bc_hi=c.bc[1], bc_value=c.bc[2],
                       by_deck=True, average_type=MODES[mode], **kw)


def _drive_reference(op, phi, rhs, out, key):
    """One residual and one relax(2) through an operator the factory made."""
    nb = range(len(op.boxes))
    fp, fr, fl = op.field(1), op.field(0, values=rhs), op.field(0)
    for n in nb:
        op.set(fp, n, phi[n], full=True)
    op.residual(fl, fp, fr, False)
    for n in nb:
        out[f"{key}/residual/{n}"] = op.get(fl, n)
        op.set(fp, n, phi[n], full=True)
    op.relax(fp, fr, 2)
    for n in nb:
        out[f"{key}/relax2/{n}"] = op.get(fp, n)


def run_reference(c, d, mode):
    """Depth 0 up to and including the first NULL.  `exists` counts the
    operators; per depth: scalars = (dx, dxCrse, alpha, beta), the valid cells
    of aCoef, bCoef and lambda, residual and relax(2)."""
    F = reference_factory(c, d, mode)
    out, depth = {}, 0
    while True:
        op = F.mg_new_op(0, depth)
        if op is None:
            break
        i = op.info()
        key = f"{c.name}/{mode}/{depth}"
        out[key + "/scalars"] = np.array([i["dx"], i["dxCrse"], i["alpha"], i["beta"]])
        for n in range(len(op.boxes)):
            out[f"{key}/a/{n}"] = op.coef(0, n, full=False)
            out[f"{key}/b/{n}"] = op.coef(1, n, full=False)
            out[f"{key}/lambda/{n}"] = op.lam(n)
        if depth < c.depths:
            _drive_reference(op, d[f"phi{depth}"], d[f"rhs{depth}"], out, key)
        depth += 1
    out[f"{c.name}/{mode}/exists"] = np.array([float(depth)])
    out[f"{c.name}/{mode}/average_type"] = np.array([float(F.average_type)])
    return out


# ------------------------------------------------------------------ the oracle
def oracle_mg(c, d, mode, boxes=None, domain=None, dx=DX):
    o = oracle.OracleMG(boxes or c.boxes, domain or c.domain, dx, alpha=ALPHA, beta=BETA,
                        periodic=c.periodic, bc_lo=c.bc[0], bc_hi=c.bc[1], bc_value=c.bc[2],
                        nlevels=-1, avg_type=restated_average(MODES[mode]))
    for n in range(o.nbox):
        o.set(0, oracle.ACOEF, n, d["a"][n])
        o.set(0, oracle.BCOEF, n, d["b"][n])
    o.setup()
    return o


def _drive_oracle(o, depth, phi, rhs, out, key):
    nb = range(o.nbox)
    for n in nb:
        o.set(depth, oracle.PHI, n, phi[n], full=True)
        o.set(depth, oracle.RHS, n, rhs[n])
    o.residual(depth, oracle.TMP, oracle.PHI, oracle.RHS, 0)
    for n in nb:
        out[f"{key}/residual/{n}"] = o.get(depth, oracle.TMP, n)
        o.set(depth, oracle.PHI, n, phi[n], full=True)
    o.relax(depth, oracle.PHI, oracle.RHS, 2)
    for n in nb:
        out[f"{key}/relax2/{n}"] = o.get(depth, oracle.PHI, n)


def run_oracle(c, d, mode, dx_crse=-1.0):
    """The same keys from oracle.OracleMG.  It keeps no dxCrse: a multigrid
    level of AMR level 0 has none, which the reference states as -1."""
    o = oracle_mg(c, d, mode)
    out = {}
    for depth in range(o.nlevels):
        key = f"{c.name}/{mode}/{depth}"
        out[key + "/scalars"] = np.array([o.dx(depth), dx_crse, ALPHA, BETA])
        for n in range(o.nbox):
            out[f"{key}/a/{n}"] = o.get(depth, oracle.ACOEF, n)
            out[f"{key}/b/{n}"] = o.get(depth, oracle.BCOEF, n)
            out[f"{key}/lambda/{n}"] = o.get(depth, oracle.LAMBDA, n)
        if depth < c.depths:
            _drive_oracle(o, depth, d[f"phi{depth}"], d[f"rhs{depth}"], out, key)
    out[f"{c.name}/{mode}/exists"] = np.array([float(o.nlevels)])
    out[f"{c.name}/{mode}/average_type"] = np.array([float(restated_average(MODES[mode]))])
    return out


# ------------------------------------------------------------------ two AMR levels
def two_level_inputs():
    t = TWO_LEVEL
    rng = np.random.default_rng(_seed(t["name"]))
    d = {}
    for l, b in enumerate((t["base"], t["patch"])):
        d[f"a{l}"] = rng.uniform(-2.0, -0.5, shape(b))
        d[f"b{l}"] = rng.uniform(0.5, 2.0, shape(b))
    for n in range(t["depths"]):
        d[f"phi{n}"] = [rng.uniform(-1, 1, shape(coarsen(t["patch"], 1 << n), 1))]
        d[f"rhs{n}"] = [rng.uniform(-1, 1, shape(coarsen(t["patch"], 1 << n)))]
    return d


def two_level_factory(d):
    t = TWO_LEVEL
    return ref.Factory([[t["base"]], [t["patch"]]], t["domain0"], DX, [[d["a0"]], [d["a1"]]],
                       [[d["b0"]], [d["b1"]]], alpha=ALPHA, beta=BETA, bc_lo=DIRI[0], bc_hi=DIRI[1],
                       bc_value=DIRI[2], by_deck=True, average_type=1)


def run_reference_two_level(d):
    """MGnewOp on the level-1 domain, depth by depth (coefficients, lambda,
    scalars), AMRnewOp of both levels (scalars, lambda) and refToFiner."""
    t, F, out = TWO_LEVEL, two_level_factory(d), {}
    depth = 0
    while True:
        op = F.mg_new_op(1, depth)
        if op is None:
            break
        i, key = op.info(), f"two-level/mg/{depth}"
        out[key + "/scalars"] = np.array([i["dx"], i["dxCrse"], i["alpha"], i["beta"]])
        out[key + "/box"] = np.array(op.boxes[0], dtype=np.float64)
        out[key + "/a/0"], out[key + "/b/0"] = op.coef(0, 0, full=False), op.coef(1, 0, full=False)
        out[key + "/lambda/0"] = op.lam(0)
        depth += 1
    out["two-level/mg/exists"] = np.array([float(depth)])
    for l in (0, 1):
        op = F.amr_new_op(l)
        i = op.info()
        out[f"two-level/amr/{l}/scalars"] = np.array([i["dx"], i["dxCrse"], i["alpha"], i["beta"]])
        out[f"two-level/amr/{l}/refs"] = np.array([float(i["refToCoarser"]), float(i["refToFiner"])])
        out[f"two-level/amr/{l}/lambda/0"] = op.lam(0)
    out["two-level/refToFiner"] = np.array([float(F.ref_to_finer(0)), float(F.ref_to_finer(1))])
    return out


def run_oracle_two_level(d):
    """oracle/amr.py's levels give dx per AMR level (dxCrse of level l is dx of
    level l - 1, -1 on level 0); the patch's multigrid chain is an OracleMG
    over the patch on the level-1 domain at that dx, as the device builds it."""
    t, out = TWO_LEVEL, {}
    A = amr.AMROracle([dict(box=t["base"], a=d["a0"], b=d["b0"]), dict(box=t["patch"], a=d["a1"], b=d["b1"])],
                      DX, t["domain0"], alpha=ALPHA, beta=BETA, bc_lo=DIRI[0], bc_hi=DIRI[1],
                      bc_value=DIRI[2], base=dict(avg_type=1))
    L0, L1 = A.L
    o = oracle.OracleMG([t["patch"]], L1.domain, L1.dx, alpha=ALPHA, beta=BETA, bc_lo=DIRI[0], bc_hi=DIRI[1],
                        bc_value=DIRI[2], nlevels=-1, avg_type=1)
    o.set(0, oracle.ACOEF, 0, d["a1"])
    o.set(0, oracle.BCOEF, 0, d["b1"])
    o.setup()
    for depth in range(o.nlevels):
        key = f"two-level/mg/{depth}"
        out[key + "/scalars"] = np.array([o.dx(depth), L0.dx, ALPHA, BETA])
        out[key + "/box"] = np.array(o.box(depth, 0), dtype=np.float64)
        out[key + "/a/0"], out[key + "/b/0"] = o.get(depth, oracle.ACOEF, 0), o.get(depth, oracle.BCOEF, 0)
        out[key + "/lambda/0"] = o.get(depth, oracle.LAMBDA, 0)
    out["two-level/mg/exists"] = np.array([float(o.nlevels)])
    for l, (lv, crse) in enumerate(((L0, -1.0), (L1, L0.dx))):
        out[f"two-level/amr/{l}/scalars"] = np.array([lv.dx, crse, lv.alpha, lv.beta])
        lam = oracle.Fab(np.zeros(lv.shape), lv.box[:3])
        oracle.lam(lam, oracle.Fab(np.ascontiguousarray(lv.a), lv.box[:3]), lv.box[:3], lv.box[3:],
                   lv.alpha, lv.beta, lv.dx)
        out[f"two-level/amr/{l}/lambda/0"] = lam.arr
    return out


# ------------------------------------------------------------------ tagging
TCase = collections.namedtuple("TCase", "name levels domains periodic thresh fields")
GROW, LATTICE = 2, (1, 4)


def _peaks(boxes, peaks, seed, floor=0.05):
    """Low noise below the threshold with chosen cells (i, j, k, value) raised."""
    rng = np.random.default_rng([20261021, 11, seed])
    out = []
    for b in boxes:
        x = rng.uniform(-floor, floor, shape(b))
        for i, j, k, v in peaks:
            if all(b[d] <= p <= b[3 + d] for d, p in enumerate((i, j, k))):
                x[k - b[2], j - b[1], i - b[0]] = v
        out.append(x)
    return out


def _tcases():
    one = [(0, 0, 0, 11, 9, 7)]
    three = [(0, 0, 0, 7, 7, 7), (8, 0, 0, 15, 7, 7), (0, 8, 0, 7, 15, 7)]
    patches = [(8, 8, 8, 15, 15, 15), (16, 8, 8, 23, 15, 15)]  # inside a 32^3 level-1 domain
    dom32 = (0, 0, 0, 31, 31, 31)
    long = [(0, 0, 0, 71, 5, 4)]
    # peaks beside the low x, the high y and the low z face; one interior; one negative
    pk_one = [(0, 4, 4, 1.0), (6, 9, 3, -0.9), (9, 2, 0, 0.8), (5, 5, 4, 0.7)]
    pk_patch = [(8, 9, 12, 1.0), (23, 15, 15, -0.8), (15, 8, 8, 0.9)]  # beside faces of the boxes
    cases = [
        TCase("one-box-clipped", [one], [one[0]], (0, 0, 0), 0.5, [_peaks(one, pk_one, 0)]),
        TCase("three-boxes", [three], [(0, 0, 0, 15, 15, 7)], (0, 0, 0), 0.5,
              [_peaks(three, [(7, 7, 3, 1.0), (8, 0, 7, -0.7), (1, 14, 0, 0.6)], 1)]),
        TCase("patches-inside", [patches], [dom32], (0, 0, 0), 0.5, [_peaks(patches, pk_patch, 2)]),
        TCase("patches-periodic", [patches], [dom32], (1, 1, 1), 0.5, [_peaks(patches, pk_patch, 2)]),
        # tags at a periodic domain's own faces: clipped, not wrapped to the far side
        TCase("periodic-domain-faces", [one], [one[0]], (1, 1, 1), 0.5, [_peaks(one, pk_one, 0)]),
        TCase("all-zero", [one], [one[0]], (0, 0, 0), 0.5, [[np.zeros(shape(one[0]))]]),
        # 0.5 * 1.0 == 0.5 exactly: the cell that holds tagVal itself is tagged (>=)
        TCase("equal-to-tagval", [one], [one[0]], (0, 0, 0), 0.5,
              [_peaks(one, [(3, 3, 3, 1.0), (8, 6, 5, 0.5), (6, 1, 2, -0.5), (0, 9, 0, 0.49999999999999994)], 3)]),
        TCase("72-long", [long], [long[0]], (0, 0, 0), 0.5,
              [_peaks(long, [(63, 2, 2, 1.0), (64, 3, 1, -1.0), (70, 0, 4, 0.75), (1, 5, 0, 0.75)], 4)]),
        # each level has its own max: 1.0 below, 40.0 above (its 0.9 peak stays untagged)
        TCase("two-levels", [one, patches], [one[0], dom32], (0, 0, 0), 0.5,
              [_peaks(one, pk_one, 5), _peaks(patches, [(8, 9, 12, 40.0), (20, 12, 10, -21.0), (12, 12, 12, 0.9)], 6)]),
    ]
    return cases


TCASES = _tcases()
TCASE = {c.name: c for c in TCASES}


def run_reference_tags(c):
    """Per level and lattice spacing, the projected tags as an ordered (n, 3) array."""
    cells = ref.tag_cells(c.levels, c.domains, c.fields, [1.0] * len(c.levels), c.thresh, GROW, c.periodic)
    out = {}
    for l, x in enumerate(cells):
        out[f"tags/{c.name}/{l}/count"] = np.array([float(len(x))])
        for s in LATTICE:
            out[f"tags/{c.name}/{l}/c{s}"] = project(x, s)
    return out


def project(cells, s):
    """Level cells onto the lattice of spacing s: floor(cell / s), each once, ordered."""
    lat = np.floor_divide(cells, s)  # the one line
    return np.unique(lat.reshape(-1, 3), axis=0).astype(np.float64)


def mask_cells(lat_lo, mask):
    """A lattice mask[z, y, x] from lat_lo as the same ordered (n, 3) array."""
    kk, jj, ii = np.nonzero(mask)
    x = np.stack([ii + lat_lo[0], jj + lat_lo[1], kk + lat_lo[2]], axis=1)
    return np.unique(x.reshape(-1, 3), axis=0).astype(np.float64)


def run_restated_tags(c):
    out = {}
    for l, (boxes, dom, vals) in enumerate(zip(c.levels, c.domains, c.fields)):
        tag_val = max(float(np.max(np.abs(v))) for v in vals) * c.thresh
        for s in LATTICE:
            lo, mask = regrid_ref.tag_lattice(vals, boxes, dom, tag_val, GROW, s)
            out[f"tags/{c.name}/{l}/c{s}"] = mask_cells(lo, mask)
        lo, mask = regrid_ref.tag_lattice(vals, boxes, dom, tag_val, GROW, 1)
        out[f"tags/{c.name}/{l}/count"] = np.array([float(mask.sum())])
    return out


# ------------------------------------------------------------------ the fixture
def build_fixture():
    """reference_factory.npz's contents, from the compiled reference: outputs only."""
    out = {}
    for c in FCASES:
        for mode in MODES:
            if mode != "deck-absent" or c.special:  # the special case's inputs do depend on the mode
                out.update(run_reference(c, finputs(c, mode), mode))
    out.update(run_reference_two_level(two_level_inputs()))
    for c in TCASES:
        out.update(run_reference_tags(c))
    return {k: digest(v) if v.size > DIGEST_ABOVE else v for k, v in out.items()}


def from_fixture(file, prefix):
    """The fixture's entries under a prefix; "<case>/deck-absent/" is held as
    "<case>/arithmetic/" unless the fixture has it."""
    out = {k: v for k, v in file.items() if k.startswith(prefix)}
    if not out and "/deck-absent/" in prefix:
        twin = prefix.replace("/deck-absent/", "/arithmetic/")
        out = {k.replace("/arithmetic/", "/deck-absent/"): v for k, v in file.items() if k.startswith(twin)}
    assert out, f"the fixture holds nothing under {prefix}"
    return out
