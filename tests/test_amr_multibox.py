"""AMR levels whose union is not a box: the multi-box restatement
oracle/amr.py MultiBoxAMROracle against the one-box AMROracle and against
known answers (CPU), and the GPU against it bit for bit -- coarse-fine
interpolation next to sibling boxes, faces that are part fine-fine and part
coarse-fine, concave corners, staging across several coarse boxes, periodic
directions with levels > 0.
"""
import itertools

import numpy as np
import pytest

from oracle.amr import AMROracle, MultiBoxAMROracle, average_down, coarsen_box

BC = dict(bc_lo=(0, 1, 0), bc_hi=(1, 0, 0), bc_value=0.125)
BASE = dict(nlevels=3, avg_type=1, prolong_type=1, bottom_solver=0)

# The L-shaped hierarchy: 16^3 base, level 1 in the 32^3 index space, level 2
# in the 64^3 one.  Three boxes per level: a slab, a second one on top of part
# of it (an L in the x-z and y-z planes, with mixed faces and concave
# corners), a third one apart from them on the x-lo domain face (Dirichlet).
# The first box of each level reaches the x-hi face (Neumann).
DOM0 = (0, 0, 0, 15, 15, 15)
DX0 = 100.0 / 16
HIER = [[DOM0],
        [(8, 8, 8, 31, 23, 15), (8, 8, 16, 15, 23, 23), (0, 8, 8, 7, 15, 15)],
        [(18, 18, 18, 63, 45, 29), (18, 18, 30, 29, 33, 45), (0, 18, 18, 13, 29, 29)]]
# two isolated level-1 patches, 2 fine cells apart diagonally (in x and y):
# no face of one touches the other, so the level takes the fused CF path
HIER_DIAG = [[DOM0], [(4, 4, 8, 13, 13, 23), (16, 16, 8, 27, 27, 23)]]
# periodic in x: level-1 boxes at both x ends (the wrap is properly nested),
# one level-2 box on the x-lo face whose coarse-fine stencils reach level 1's
# cells at the far x end
PERIODIC = (1, 0, 0)
HIER_PER = [[DOM0],
            [(0, 8, 8, 15, 23, 15), (0, 8, 16, 7, 23, 23), (24, 8, 8, 31, 23, 23)],
            [(0, 18, 18, 21, 45, 29), (0, 18, 30, 13, 33, 45)]]
HIER_PER_BAD = [HIER_PER[0], HIER_PER[1][:2], HIER_PER[2]]  # nothing at the far x end


def _shape(b):
    return (b[5] - b[2] + 1, b[4] - b[1] + 1, b[3] - b[0] + 1)


def _data(rng, hier, bvar=True):
    out = []
    for boxes in hier:
        ss = [_shape(b) for b in boxes]
        out.append(dict(boxes=list(boxes), a=[rng.uniform(-2.0, -0.5, s) for s in ss],
                        b=[rng.uniform(0.5, 2.0, s) if bvar else np.ones(s) for s in ss],
                        rhs=[rng.uniform(-1, 1, s) for s in ss]))
    return out


def _oracle(lv, periodic=(0, 0, 0), dx0=DX0, dom0=DOM0, **kw):
    return MultiBoxAMROracle(lv, dx0, dom0, alpha=1.0, beta=-1.0, **BC, base=BASE,
                             periodic=periodic, **kw)


def _flat(lv, key):
    return [x for level in lv for x in level[key]]


def _maxnorm(res):
    return max(np.abs(r).max() for r in res)


# ----------------------------------------------------- geometry, from the boxes
def _mask(boxes, n):
    m = np.zeros((n,) * 3, bool)  # indexed [x, y, z]
    for b in boxes:
        assert not m[b[0]:b[3] + 1, b[1]:b[4] + 1, b[2]:b[5] + 1].any(), "boxes overlap"
        m[b[0]:b[3] + 1, b[1]:b[4] + 1, b[2]:b[5] + 1] = True
    return m


def _ghosts(boxes, n, periodic=(0, 0, 0)):
    """every ghost cell of every non-domain face: (box, dir, side, cell,
    inside the level?, usable flags of the 4 tangential coarse neighbours
    (-d0, +d0, -d1, +d1), of the 4 diagonals)"""
    fm, cov, nc = _mask(boxes, n), _mask([coarsen_box(b) for b in boxes], n // 2), n // 2

    def usable(q):
        q = list(q)
        for d in range(3):
            if periodic[d]:
                q[d] %= nc
            elif not 0 <= q[d] < nc:
                return False
        return not cov[tuple(q)]

    for bi, b in enumerate(boxes):
        for d in range(3):
            t = [e for e in range(3) if e != d]
            for side in (0, 1):
                if not periodic[d] and (b[3 + d] == n - 1 if side else b[d] == 0):
                    continue
                for p0 in range(b[t[0]], b[3 + t[0]] + 1):
                    for p1 in range(b[t[1]], b[3 + t[1]] + 1):
                        g = [0, 0, 0]
                        g[d], g[t[0]], g[t[1]] = (b[3 + d] + 1 if side else b[d] - 1), p0, p1
                        gc = [v // 2 for v in g]
                        nb, dg = [], []
                        for e in t:
                            for s in (-1, 1):
                                q = list(gc)
                                q[e] += s
                                nb.append(usable(q))
                        for s0, s1 in itertools.product((-1, 1), repeat=2):
                            q = list(gc)
                            q[t[0]] += s0
                            q[t[1]] += s1
                            dg.append(usable(q))
                        yield bi, d, side, tuple(g), bool(fm[tuple(v % n for v in g)]), nb, dg


def _stats(boxes, n, periodic=(0, 0, 0)):
    kinds, owners = {}, {}
    cov = _mask([coarsen_box(b) for b in boxes], n // 2)
    one_sided = covered_tangential = diag_only = 0
    for bi, d, side, g, inside, nb, dg in _ghosts(boxes, n, periodic):
        kinds.setdefault((bi, d, side), set()).add(inside)
        if inside:
            continue
        owners.setdefault(g, set()).add(d)
        gc = [v // 2 for v in g]
        t = [e for e in range(3) if e != d]
        for e in t:  # a tangential coarse neighbour inside the domain that the level covers
            for s in (-1, 1):
                q = list(gc)
                q[e] += s
                if all(0 <= v < n // 2 for v in q) and cov[tuple(q)]:
                    covered_tangential += 1
        if not all(nb):
            one_sided += 1
        elif not all(dg):
            diag_only += 1
    return dict(mixed_faces=sum(1 for k in kinds.values() if len(k) == 2),
                two_dir_ghosts=sum(1 for v in owners.values() if len(v) > 1),
                one_sided=one_sided, covered_tangential=covered_tangential, diag_only=diag_only)


def _is_box(boxes):
    lo = [min(b[d] for b in boxes) for d in range(3)]
    hi = [max(b[3 + d] for b in boxes) for d in range(3)]
    vol = sum(int(np.prod([b[3 + d] - b[d] + 1 for d in range(3)])) for b in boxes)
    return vol == int(np.prod([h - l + 1 for l, h in zip(lo, hi)]))


def _nested(fine, coarse, nc, periodic=(0, 0, 0)):
    cm = _mask(coarse, nc)
    for b in fine:
        c = coarsen_box(b)
        rng = []
        for d in range(3):
            r = range(c[d] - 1, c[3 + d] + 2)
            rng.append([v % nc for v in r] if periodic[d] else [v for v in r if 0 <= v < nc])
        if not cm[np.ix_(*rng)].all():
            return False
    return True


def test_hierarchy_properties():
    for hier, per in ((HIER, (0, 0, 0)), (HIER_PER, PERIODIC)):
        for l in range(1, len(hier)):
            assert _nested(hier[l], hier[l - 1], 16 << (l - 1), per), l
    assert not _nested(HIER_PER_BAD[2], HIER_PER_BAD[1], 32, PERIODIC)
    # (clipped to the domain, as csrc/amr.cpp did, the bad hierarchy passes)
    assert _nested(HIER_PER_BAD[2], HIER_PER_BAD[1], 32, (0, 0, 0))
    want = {1: dict(mixed_faces=2, two_dir_ghosts=32, diag_only=4),
            2: dict(mixed_faces=1, two_dir_ghosts=28, diag_only=4)}
    for l in (1, 2):
        assert not _is_box(HIER[l])
        s = _stats(HIER[l], 16 << l)
        assert s["mixed_faces"] >= 1 and s["two_dir_ghosts"] >= 1
        assert s["covered_tangential"] >= 1 and s["one_sided"] >= 1 and s["diag_only"] >= 1
        for k, v in want[l].items():
            assert s[k] == v, (l, s)
    # a box on a Dirichlet face (x lo) and one on a Neumann face (x hi)
    for l in (1, 2):
        n = 16 << l
        assert BC["bc_lo"][0] == 0 and any(b[0] == 0 for b in HIER[l])
        assert BC["bc_hi"][0] == 1 and any(b[3] == n - 1 for b in HIER[l])
    # the diagonal patches: isolated (no face ghost of one inside the other)
    assert all(not inside for *_, inside, _, _ in _ghosts(HIER_DIAG[1], 32))
    # the periodic hierarchy: a CF ghost whose stencil wraps to the far x end
    s = _stats(HIER_PER[2], 64, PERIODIC)
    assert s["mixed_faces"] >= 1 and s["one_sided"] >= 1
    wraps = 0
    for bi, d, side, g, inside, nb, dg in _ghosts(HIER_PER[2], 64, PERIODIC):
        if not inside and d != 0 and g[0] // 2 == 0 and nb[0]:
            wraps += 1  # its -x coarse neighbour (nb[0]) is cell 31 of level 1, usable
    assert wraps >= 1


# ------------------------------------------------------------ split invariance
ONE_DOM0 = (0, 0, 0, 31, 31, 31)
ONE_BOXES = [ONE_DOM0, (8, 16, 12, 47, 41, 45), (30, 40, 36, 73, 71, 77)]


def _cut(b):
    """2 x 2 x 1 boxes (cuts at even indices)"""
    mx = b[0] + ((b[3] - b[0] + 1) // 4) * 2
    my = b[1] + ((b[4] - b[1] + 1) // 4) * 2
    return [(x0, y0, b[2], x1, y1, b[5]) for y0, y1 in ((b[1], my - 1), (my, b[4]))
            for x0, x1 in ((b[0], mx - 1), (mx, b[3]))]


def _sub(arr, b, part):
    return arr[part[2] - b[2]:part[5] - b[2] + 1, part[1] - b[1]:part[4] - b[1] + 1,
               part[0] - b[0]:part[3] - b[0] + 1].copy()


def test_split_invariance_bitwise():
    rng = np.random.default_rng(11)
    one, multi = [], []
    for l, b in enumerate(ONE_BOXES):
        s = _shape(b)
        d = dict(box=b, a=rng.uniform(-2.0, -0.5, s), b=rng.uniform(0.5, 2.0, s),
                 rhs=rng.uniform(-1, 1, s))
        one.append(d)
        parts = [b] if l == 0 else _cut(b)
        multi.append(dict(boxes=parts, **{k: [_sub(d[k], b, p) for p in parts]
                                          for k in ("a", "b", "rhs")}))
    dx0 = 100.0 / 32
    o1 = AMROracle(one, dx0, ONE_DOM0, alpha=1.0, beta=-1.0, **BC, base=BASE)
    om = _oracle(multi, dx0=dx0, dom0=ONE_DOM0)
    assert [len(ix) for ix in om.ix] == [1, 4, 4]
    r1 = o1.init_residual([lv.full() for lv in o1.L], [x["rhs"] for x in one])
    rm = om.init_residual(om.zeros_ml(), _flat(multi, "rhs"))
    assert _maxnorm(r1) == _maxnorm(rm)
    for _ in range(3):
        r1, rm = o1.iteration(), om.iteration()
        assert _maxnorm(r1) == _maxnorm(rm)
    for l, b in enumerate(ONE_BOXES):
        for bx, got, res in zip(om.B[l], om.lv(om.phis, l), om.lv(rm, l)):
            assert np.array_equal(got[1:-1, 1:-1, 1:-1],
                                  _sub(o1.phis[l][1:-1, 1:-1, 1:-1], b, bx.box)), (l, bx.box)
            assert np.array_equal(res, _sub(r1[l], b, bx.box)), (l, bx.box)


# ---------------------------------------------------------------- known answer
def _centres(b, dx):
    z, y, x = np.meshgrid(*[(np.arange(b[d] - 1, b[3 + d] + 2) + 0.5) * dx for d in (2, 1, 0)],
                          indexing="ij")
    return x, y, z


@pytest.mark.parametrize("cxy", [0.0, 0.011], ids=["linear", "xy"])
def test_cf_interp_known_answer(cxy):
    """the stencil weights and offsets, independently of the kernel: a linear
    field is reproduced at every CF ghost (centred, one-sided, mixed term
    dropped alike); with an xy term at every one that has a usable neighbour
    in both tangential directions and all four diagonals"""
    def f(x, y, z):
        return 1.3 * x - 0.7 * y + 0.45 * z + 2.0 + cxy * x * y

    rng = np.random.default_rng(12)
    o = _oracle(_data(rng, HIER))
    checked = 0
    for l in (1, 2):
        dxf, dxc = DX0 / 2 ** l, DX0 / 2 ** (l - 1)
        cs = [bx.full() for bx in o.B[l - 1]]
        for bx, c in zip(o.B[l - 1], cs):
            c[...] = f(*_centres(bx.box, dxc))
        us, want = [], []
        for bx in o.B[l]:
            w = f(*_centres(bx.box, dxf))
            want.append(w)
            us.append(bx.full(w[1:-1, 1:-1, 1:-1]))
        o.cf_interp(l, us, cs)
        scale = max(np.abs(w).max() for w in want)
        for bi, d, side, g, inside, nb, dg in _ghosts(HIER[l], 16 << l):
            if inside:
                continue
            if cxy and not ((nb[0] or nb[1]) and (nb[2] or nb[3]) and all(dg)):
                continue
            b = HIER[l][bi]
            idx = tuple(g[e] - b[e] + 1 for e in (2, 1, 0))
            assert abs(us[bi][idx] - want[bi][idx]) <= 1e-13 * scale, (l, bi, d, side, g)
            checked += 1
    assert checked > 1000


# ------------------------------------------------------- convergence, the solve
def test_multibox_vcycle_converges():
    rng = np.random.default_rng(2)
    lv = _data(rng, HIER)
    o = _oracle(lv)
    hist = [_maxnorm(o.init_residual(o.zeros_ml(), _flat(lv, "rhs")))]
    for _ in range(4):
        hist.append(_maxnorm(o.iteration()))
    assert hist[-1] < 1e-3 * hist[0], hist
    assert all(b < a for a, b in zip(hist, hist[1:])), hist


SOLVE_SEED, SOLVE_EPS = 23, 1e-10


def _solve_case(dot_fsum):
    rng = np.random.default_rng(SOLVE_SEED)
    lv = _data(rng, HIER, bvar=False)
    o = _oracle(lv, dot_fsum=dot_fsum)
    phis = o.zeros_ml()
    it, nrm = o.solve(phis, o.full_ml(_flat(lv, "rhs")), num_mg_iterations=2, imax=20,
                      eps=SOLVE_EPS)
    return lv, o, phis, it, nrm


@pytest.fixture(scope="module")
def solve_ref():
    return _solve_case(False)


def test_solve_insensitive_to_summation_order(solve_ref):
    # The dot products summed per box and then over boxes, against math.fsum
    # over all cells of a level: any order the GPU reduces in lies between.
    # Observed for SOLVE_SEED / SOLVE_EPS: both take 2 iterations (two V-cycles
    # per preconditioning reduce the residual by ~1e-6 per iteration) and phi
    # differs by rel-L2 3.5e-19, so the GPU comparison can ask for equal
    # iteration counts and 1e-10 (the bicg_cases convention).
    _, _, pa, ita, _ = solve_ref
    _, _, pb, itb, _ = _solve_case(True)
    assert ita == itb and 2 <= ita < 20
    num = np.sqrt(sum(np.sum((a - b) ** 2) for a, b in zip(pa, pb)))
    den = np.sqrt(sum(np.sum(a ** 2) for a in pa))
    print("solve sensitivity: iterations", ita, "rel-L2", num / den)
    assert num <= 1e-12 * den, num / den


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def comm():
    import mg_ic_code_amd as mg
    return mg.Comm()


class _Dev:
    """the hierarchy on the device; fields are one LevelData per level, host
    data the restatement's flat per-box lists"""

    def __init__(self, comm, lv, periodic=(0, 0, 0)):
        import mg_ic_code_amd as mg
        self.mg = mg
        self.grids, self.order, levels = [], [], []
        dom, dx = DOM0, DX0
        for l, x in enumerate(lv):
            grid = mg.Grid(comm, dom, x["boxes"], dx, periodic=periodic, patches=l > 0)
            # local box k is box order[k] of the level's list
            self.order.append([x["boxes"].index(grid.local_box(k))
                               for k in range(grid.num_local)])
            assert sorted(self.order[-1]) == list(range(len(x["boxes"])))
            self.grids.append(grid)
            dom = tuple(2 * v if i < 3 else 2 * v + 1 for i, v in enumerate(dom))
            dx /= 2
        self.a = self.field(_flat(lv, "a"))
        self.b = self.field(_flat(lv, "b"))
        self.rhs = self.field(_flat(lv, "rhs"))
        self.phi = self.field()
        op = mg.OperatorParams(alpha=1.0, beta=-1.0, coefficient_average_type=1, prolong_type=1,
                               **BC)
        self.amr = mg.AMRSolver(list(zip(self.grids, self.a, self.b)), op,
                                mg.SolverParams(max_depth=2, bottom_solver=0))

    def split(self, flat):
        out, n = [], 0
        for o in self.order:
            out.append(flat[n:n + len(o)])
            n += len(o)
        return out

    def up(self, fields, flat, levels=None):
        """valid cells from per-box arrays (valid, or full: ghosts dropped)"""
        for l, (f, arrs) in enumerate(zip(fields, self.split(flat))):
            if levels is not None and l not in levels:
                continue
            for k, i in enumerate(self.order[l]):
                a, s = arrs[i], _shape(self.grids[l].local_box(k))
                f.upload(k, a if a.shape == s else a[1:-1, 1:-1, 1:-1])

    def field(self, flat=None):
        fs = [self.mg.LevelData(g) for g in self.grids]
        if flat is None:
            for f in fs:
                f.set_zero()
        else:
            self.up(fs, flat)
        return fs

    def down(self, f, l, with_ghosts=False):
        out = [None] * len(self.order[l])
        for k, i in enumerate(self.order[l]):
            out[i] = f.download(k, with_ghosts=with_ghosts)
        return out

    def down_all(self, fs):
        return [x for l, f in enumerate(fs) for x in self.down(f, l)]


def _random_ml(rng, o):
    return [b.full(rng.uniform(-1, 1, b.shape)) for bs in o.B for b in bs]


def _faces_equal(o, l, got, want, tag):
    """the ghosts of every non-domain face of every box (edges and corners
    are no ghost of the 7-point stencil)"""
    n = 0
    for i, (bx, g, w) in enumerate(zip(o.B[l], got, want)):
        for dir in range(3):
            for side in (0, 1):
                if bx.domain_face(dir, side):
                    continue
                sl = [slice(1, -1)] * 3
                sl[2 - dir] = -1 if side else 0
                assert np.array_equal(g[tuple(sl)], w[tuple(sl)]), (tag, l, i, dir, side)
                n += 1
    return n


CASES = {"lshape": (HIER, (0, 0, 0)), "periodic": (HIER_PER, PERIODIC)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_cf_interp_every_box_and_face_bitwise(comm, case):
    hier, per = CASES[case]
    rng = np.random.default_rng(31)
    lv = _data(rng, hier)
    dev, o = _Dev(comm, lv, per), _oracle(lv, per)
    us = _random_ml(rng, o)
    f = dev.field(us)
    for l in range(1, len(hier)):
        for coarse in (True, False):
            dev.up(f, us, levels=(l,))
            dev.amr.cf_interp(l, f[l], f[l - 1] if coarse else None)
            U = [u.copy() for u in o.lv(us, l)]
            o.cf_interp(l, U, o.lv(us, l - 1) if coarse else None)
            # every ghost of every non-domain face after cf_interp alone (it
            # writes whole faces: the CF cells and the ones a sibling covers)
            assert _faces_equal(o, l, dev.down(f[l], l, True), U, (case, coarse, "cf")) > 6
            # the sibling-covered part of the mixed faces after the exchange
            # that follows in AMROperator; the CF cells stay
            f[l].exchange()
            o.exchange(l, U)
            _faces_equal(o, l, dev.down(f[l], l, True), U, (case, coarse, "exchange"))


@pytest.mark.gpu
@pytest.mark.parametrize("bvar", [False, True], ids=["bconst", "bvar"])
def test_level_operators_bitwise(comm, bvar):
    rng = np.random.default_rng(32)
    lv = _data(rng, HIER, bvar)
    dev, o = _Dev(comm, lv), _oracle(lv)
    us, rs = _random_ml(rng, o), _random_ml(rng, o)
    fu, fr, fout, fc = dev.field(us), dev.field(rs), dev.field(), dev.field()
    amr = dev.amr
    for l in (1, 2):
        def U():
            return [u.copy() for u in o.lv(us, l)]

        C = o.lv(us, l - 1)
        R = [r[1:-1, 1:-1, 1:-1] for r in o.lv(rs, l)]
        for hom in (False, True):
            # AMROperator: CF ghosts from level l - 1, exchange, physical BC
            dev.up(fu, us, levels=(l,))
            amr.AMROperator(l, fout[l], fu[l], fu[l - 1], hom)
            u = U()
            o.fill(l, u, C, hom)
            for i, (bx, got) in enumerate(zip(o.B[l], dev.down(fout[l], l))):
                assert np.array_equal(got, -bx.residual(u[i], np.zeros(bx.shape))), (l, hom, i)
            dev.up(fu, us, levels=(l,))
            amr.AMRResidual(l, fout[l], fu[l], fu[l - 1], fr[l], hom)
            want = o.amr_residual(l, U(), C, R, hom)
            for i, got in enumerate(dev.down(fout[l], l)):
                assert np.array_equal(got, want[i]), (l, hom, i)
        # AMRRestrict: average(r - L(u)) (homogeneous CF) onto the covered cells
        # of level l - 1 (for l = 2 across its three boxes), the others untouched
        dev.up(fu, us, levels=(l,))
        dev.up(fc, us, levels=(l - 1,))
        amr.AMRRestrict(l, fc[l - 1], fr[l], fu[l], None)
        want = [c[1:-1, 1:-1, 1:-1].copy() for c in C]
        before = [w.copy() for w in want]
        o.put_covered(l, want, [average_down(x) for x in o.amr_residual(l, U(), None, R, True)])
        assert any(not np.array_equal(a, b) for a, b in zip(want, before))
        assert any((a == b).any() for a, b in zip(want, before))  # uncovered cells exist
        for i, got in enumerate(dev.down(fc[l - 1], l - 1)):
            assert np.array_equal(got, want[i]), (l, i)
        # AMRProlong: piecewise constant, staged from the coarse boxes
        dev.up(fu, us, levels=(l,))
        amr.AMRProlong(l, fu[l], fu[l - 1])
        u = U()
        o.prolong_const(l, u, C)
        for i, got in enumerate(dev.down(fu[l], l)):
            assert np.array_equal(got, u[i][1:-1, 1:-1, 1:-1]), (l, i)
        # AMRUpdateResidual: r - L(u), CF ghosts of u from level l - 1
        dev.up(fu, us, levels=(l,))
        dev.up(fr, rs, levels=(l,))
        amr.AMRUpdateResidual(l, fr[l], fu[l], fu[l - 1])
        want = o.amr_residual(l, U(), C, R, True)
        for i, got in enumerate(dev.down(fr[l], l)):
            assert np.array_equal(got, want[i]), (l, i)
        dev.up(fr, rs, levels=(l,))


VCYCLES = {"lshape": (HIER, (0, 0, 0)), "diagonal": (HIER_DIAG, (0, 0, 0)),
           "periodic": (HIER_PER, PERIODIC)}


@pytest.mark.gpu
@pytest.mark.parametrize("bvar", [False, True], ids=["bconst", "bvar"])
@pytest.mark.parametrize("case", ["lshape", "diagonal", "periodic"])
def test_vcycle_bitwise(comm, case, bvar):
    hier, per = VCYCLES[case]
    rng = np.random.default_rng(33)
    lv = _data(rng, hier, bvar)
    dev, o = _Dev(comm, lv, per), _oracle(lv, per)
    res = o.init_residual(o.zeros_ml(), _flat(lv, "rhs"))
    g0 = dev.amr.init_residual(dev.phi, dev.rhs, 0)
    assert g0 == _maxnorm(res)
    for _ in range(3):
        g = dev.amr.iteration(dev.phi, dev.rhs, 0)
        assert g == _maxnorm(o.iteration())
    for l in range(len(hier)):
        for i, (got, want) in enumerate(zip(dev.down(dev.phi[l], l), o.lv(o.phis, l))):
            assert np.array_equal(got, want[1:-1, 1:-1, 1:-1]), (l, i)
    assert g < 0.2 * g0


@pytest.mark.gpu
def test_multilevel_op_bitwise_and_reductions(comm):
    rng = np.random.default_rng(34)
    lv = _data(rng, HIER, bvar=False)
    dev, o = _Dev(comm, lv), _oracle(lv)
    amr = dev.amr
    xs = _random_ml(rng, o)
    fx, fl = dev.field(xs), dev.field()
    amr.applyOp(fl, fx, True)
    want = o.apply_op([x.copy() for x in xs], True)
    for i, got in enumerate(dev.down_all(fl)):
        assert np.array_equal(got, want[i][1:-1, 1:-1, 1:-1]), i
    # dot / norms: reductions in another order
    assert amr.dotProduct(fl, fx) == pytest.approx(o.dot(want, xs), rel=1e-12)
    masked = o.masked(xs)
    assert any(not np.array_equal(m, x) for m, x in zip(masked, xs))
    for ord_ in (0, 1, 2):
        assert amr.norm(fl, ord_) == pytest.approx(o.norm(want, ord_), rel=1e-12)
        assert amr.computeNorm(fx, ord_) == pytest.approx(o.norm(masked, ord_), rel=1e-12)
    assert amr.computeSum(fx) == pytest.approx(
        sum(o.weight(l) * sum(float(m[1:-1, 1:-1, 1:-1].sum()) for m in o.lv(masked, l))
            for l in range(3)), rel=1e-11)
    # the preconditioner on a composite residual (covered cells zero)
    r = o.residual_ml(o.zeros_ml(), o.full_ml(_flat(lv, "rhs")))
    fr, fe = dev.field(r), dev.field()
    amr.precondition(fe, fr, 2)
    e = o.precondition(r, 2)
    for i, got in enumerate(dev.down_all(fe)):
        assert np.array_equal(got, e[i][1:-1, 1:-1, 1:-1]), i


@pytest.mark.gpu
def test_multilevel_bicgstab_solve_matches_restatement(comm, solve_ref):
    import mg_ic_code_amd as mg
    lv, o, phis, it_o, nrm_o = solve_ref
    dev = _Dev(comm, lv)
    solver = mg.BiCGStabSolver(mg.MultilevelLinearOp(dev.amr, 2), tolerance=SOLVE_EPS,
                               max_iterations=20, norm_type=0)
    it = solver.solve(dev.phi, dev.rhs)
    assert it == it_o
    assert solver.final_norm == pytest.approx(nrm_o, rel=1e-6, abs=1e-14)
    got = dev.down_all(dev.phi)
    num = np.sqrt(sum(np.sum((g - w[1:-1, 1:-1, 1:-1]) ** 2) for g, w in zip(got, phis)))
    den = np.sqrt(sum(np.sum(w[1:-1, 1:-1, 1:-1] ** 2) for w in phis))
    print("solve: iterations", it, "rel-L2", num / den)
    assert num <= 1e-10 * den
    for g, w in zip(got, phis):  # and box by box
        assert np.linalg.norm(g - w[1:-1, 1:-1, 1:-1]) <= 1e-10 * np.linalg.norm(w), g.shape


@pytest.mark.gpu
def test_periodic_level_not_nested_through_the_wrap_is_rejected(comm):
    # level 2 touches the periodic x-lo face; its coarse-fine stencils read
    # level 1 at the far x end, where this hierarchy has nothing
    from mg_ic_code_amd._lib import MgicError
    rng = np.random.default_rng(35)
    with pytest.raises(MgicError) as e:
        _Dev(comm, _data(rng, HIER_PER_BAD), PERIODIC)
    assert e.value.code < 0 and "nested" in str(e.value)
    _Dev(comm, _data(rng, HIER_PER), PERIODIC)  # with the far end: accepted
