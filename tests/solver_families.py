"""Seeded inputs for the solver tests (test_solvers_exact_{cpu,gpu}.py) where a double-precision walk can go wrong,
each reduced with list_helpers.lll_exact (rational arithmetic): nothing here depends on the code under test.

  scaled_root  s B0 with one to three extra columns in [-3, 3] (and s B0 + E, E a full perturbation in [-3, 3]); B0 the
               reduced D4 and 2 E8 bases, s = 2^10, 2^20, 2^27, 2^29.  The 24 (240) minimal vectors of B0 become
               near-ties whose integer norms s^2 |x B0|^2 + (x e)^2 differ by 0, 1, 4, ... at a magnitude up to 2^61,
               where neither the norms nor the Gram entries are doubles.
  knapsack     [I_d | a], a of 30 and of 40 bits, d = 12, 16, 20: a skewed, non-q-ary profile, entries of mixed size.
  wide         d = 12 with n = 64, 65, 130, 200, 256 columns of 20-bit entries: one per columns-per-lane class.
  cut_rows     last rows long enough for last_useful_index to cut them (d_eff < d), the boundary r_ii = 2 r_00 (kept)
               and 2 r_00 + 1 (cut) on an orthogonal tail where the doubles are exact, and a basis whose rows have
               entries of very different sizes (row exponents far apart) with the shortest vector in the last row.
  lane_edge    d = 63, 64: 40 on the diagonal, the answer needs the coefficient of the last row (lane d - 1).

MEMBERS: name -> (family, thunk); basis(name) -> [d][n] Python integers, computed once per process (read-only).
Size condition of every member (asserted in test_solvers_exact_cpu.py): exact_lattice.short_exact at
N = (norm of the shortest row) - 1 visits at most NODE_CAP nodes.
"""
import numpy as np

import list_helpers as H

NODE_CAP = 200_000
SCALES = (10, 20, 27, 29)


def _py(b):
    return [[int(v) for v in row] for row in b]


def root_basis(which):
    return H.d4_basis() if which == "d4" else H.lll_exact(H.e8_basis()[0])


def scaled_root(which, log_s, extra, seed):
    """s B0 | E with E [d][extra] in [-3, 3]; extra = 0: s B0 + E with E [d][d]."""
    b0 = np.array(root_basis(which), dtype=object)
    d = b0.shape[0]
    rng = np.random.default_rng(1000 * log_s + 10 * seed + extra + (500 if which == "e8" else 0))
    s = 1 << log_s
    if extra:
        e = rng.integers(-3, 4, size=(d, extra))
        b = [[s * int(v) for v in b0[i]] + [int(v) for v in e[i]] for i in range(d)]
    else:
        e = rng.integers(-3, 4, size=(d, d))
        b = [[s * int(b0[i][j]) + int(e[i][j]) for j in range(d)] for i in range(d)]
    return H.lll_exact(b)


def scaled_root_minimum(which, log_s, reduced):
    """The exact minimum of a scaled_root member with extra columns, without enumerating at that scale: the minimum of
    s^2 m + |x E|^2 over the minimal vectors x B0 of B0 (any other lattice vector has |x B0|^2 >= m + 2, D4 and 2 E8
    being even — times 4 for 2 E8 — so it is longer by at least 2 s^2 - (the extra columns' share) > 0).  Computed on
    the reduced basis: the norms of all lattice vectors whose first d0 columns form a minimal vector of s B0."""
    import exact_lattice as X
    b0 = root_basis(which)
    d0 = len(b0[0])
    s = 1 << log_s
    head = [[v // s for v in row[:d0]] for row in reduced]  # the root lattice in the reduced basis' coordinates
    assert all(v % s == 0 for row in reduced for v in row[:d0])
    m, xs, _ = X.lambda1_exact(head)
    norms = sorted(sum(v * v for v in X.vector_of(reduced, x)) for x in xs)
    assert all(nv // (s * s) == m for nv in norms)
    return norms


def knapsack(d, bits, seed):
    rng = np.random.default_rng(100 * d + bits + 7 * seed)
    a = [int(rng.integers(1 << (bits - 1), 1 << bits)) for _ in range(d)]
    return H.lll_exact([[int(i == j) for j in range(d)] + [a[i]] for i in range(d)])


def wide(n, seed=0):
    rng = np.random.default_rng(12 * n + seed)
    return H.lll_exact(_py(rng.integers(-(1 << 20) + 1, 1 << 20, size=(12, n))))


def _cut_top():
    return [[10, 1, 0, 0, 1, 0], [0, 10, 1, 0, 0, 1], [1, 0, 10, 1, 0, 0], [0, 1, 0, 10, 1, 0]]


def cut_scaled():
    """The last two rows 2^20 times longer than the first four (test_rows_cut_by_last_useful_index's basis), reduced:
    d_eff = 4 of 6."""
    return H.lll_exact(_cut_top() + [[(1 << 20) * v for v in row] for row in ([1, -2, 0, 3, 5, 1], [2, 0, -1, 1, 1, 4])])


def cut_boundary(kept):
    """Orthogonal rows: b_0 = (12, 12, 0 ...) has r_00 = 288, three rows of norm 225 .. 250 follow, and the last row
    is (.., 24, 0) with r = 576 = 2 r_00 exactly (kept: d_eff = 5) or (.., 24, 1) with r = 577 (cut: d_eff = 4).
    Every mu is 0 and every r an integer: the doubles are exact whatever computes them."""
    b = [[12, 12, 0, 0, 0, 0, 0, 0], [0, 0, 15, 0, 0, 0, 0, 0], [0, 0, 0, 15, 4, 0, 0, 0], [0, 0, 0, 0, 0, 15, 0, 0]]
    return b + [[0, 0, 0, 0, 0, 0, 24, 0 if kept else 1]]


def cut_expo_skew():
    """Orthogonal rows whose entries differ in size while their norms fall: (64, 0 ..) r = 4096, (0, 40, 40, 0 ..)
    r = 3200, (0, 0, 0, 31, 31, 31) r = 2883.  Every row is useful (d_eff = 3) and the last is the shortest; the
    STORED r_ii of a GSO with row exponents 7, 6, 5 are 0.25, 0.78, 2.8: compared without the exponents, rows 1 and 2
    would be cut."""
    return [[64, 0, 0, 0, 0, 0], [0, 40, 40, 0, 0, 0], [0, 0, 0, 31, 31, 31]]


def steep(d):
    """tests/test_svp_solver_gpu.py's _steep(d), the same numbers."""
    rng = np.random.default_rng(d)
    b = np.diag([40 + (i % 5) for i in range(d)]).astype(np.int64) + rng.integers(-1, 2, size=(d, d))
    b[d - 2, d - 2] = 37
    b[d - 2] += b[d - 1]
    return _py(b)


def _members():
    m = {}
    # extra columns 1, 2, 3 and the full perturbation (0), spread over the scales; both roots at the largest scale
    for which, log_s, extra, seed in (("d4", 10, 1, 0), ("d4", 20, 2, 0), ("d4", 27, 3, 0), ("d4", 29, 1, 1),
                                      ("e8", 10, 2, 0), ("e8", 20, 3, 0), ("e8", 27, 1, 0), ("e8", 29, 2, 0),
                                      ("e8", 29, 3, 1), ("d4", 29, 0, 0), ("e8", 20, 0, 0), ("e8", 29, 0, 0)):
        name = "root_%s_s%d_%s%d" % (which, log_s, "x%d_" % extra if extra else "full_", seed)
        m[name] = ("scaled_root", (lambda w=which, l=log_s, e=extra, s=seed: scaled_root(w, l, e, s)),
                   dict(which=which, log_s=log_s, extra=extra))
    for d, bits, seed in ((12, 30, 0), (16, 30, 0), (20, 30, 0), (12, 40, 0), (16, 40, 0), (20, 40, 0)):
        m["knap_d%d_b%d" % (d, bits)] = ("knapsack", (lambda d=d, b=bits, s=seed: knapsack(d, b, s)), {})
    for n in (64, 65, 130, 200, 256):
        m["wide_n%d" % n] = ("wide", (lambda n=n: wide(n)), {})
    m["cut_scaled"] = ("cut_rows", cut_scaled, {})
    m["cut_kept"] = ("cut_rows", lambda: cut_boundary(True), {})
    m["cut_cut"] = ("cut_rows", lambda: cut_boundary(False), {})
    m["cut_expo_skew"] = ("cut_rows", cut_expo_skew, {})
    for d in (63, 64):
        m["steep_%d" % d] = ("lane_edge", (lambda d=d: steep(d)), {})
    return m


MEMBERS = _members()
_cache = {}


def basis(name):
    if name not in _cache:
        _cache[name] = _py(MEMBERS[name][1]())
    return _cache[name]


def family(name):
    return MEMBERS[name][0]


def info(name):
    return MEMBERS[name][2]


def names(*families):
    return [k for k, v in MEMBERS.items() if not families or v[0] in families]


# ---- the exact answers, computed once per process and shared (read-only) ---------------------------------------------
_exact = {}


def exact(name):
    """dict(N0: the shortest row's norm, d_eff, lam1, minimal: the set of all minimal coefficient vectors of the first
    d_eff rows, both signs, padded with zeros to d; i0: the first row of norm N0 below d_eff; cap_nodes: short_exact's
    node count at N0 - 1 (the size condition))."""
    import exact_lattice as X
    if name not in _exact:
        b = basis(name)
        d = len(b)
        de = X.d_eff_exact(b)
        rn = [sum(v * v for v in row) for row in b]
        N0 = min(rn[:de])
        lam1, xs, _ = X.lambda1_exact(b, rows=de)
        pad = (0,) * (d - de)
        minimal = {tuple(x) + pad for x in xs} | {tuple(-v for v in x) + pad for x in xs}
        _, cap_nodes = X.short_exact(b, min(rn) - 1, max_nodes=2 * NODE_CAP)
        _exact[name] = dict(N0=N0, d_eff=de, lam1=lam1, minimal=minimal, i0=rn.index(N0), cap_nodes=cap_nodes)
    return _exact[name]


def norms_exact(name, how_many=3):
    """The first `how_many` distinct squared norms of the lattice and short_exact's list up to the last of them."""
    import exact_lattice as X
    key = ("norms", name, how_many)
    if key not in _exact:
        b = basis(name)
        N = exact(name)["lam1"]
        while True:  # (grow the bound until it holds enough distinct norms; the lists stay small on these members)
            lst, _ = X.short_exact(b, N, max_nodes=NODE_CAP)
            distinct = sorted({nv for nv, _ in lst})
            if len(distinct) >= how_many:
                break
            N = N + max(1, N // 4)
        keep = distinct[:how_many]
        _exact[key] = (keep, [(nv, x) for nv, x in lst if nv <= keep[-1]])
    return _exact[key]


def _even_combination(b):
    """A 0/1 coefficient vector x != 0 (at most 12 rows searched) with every entry of x b even, or None: x b / 2 is then
    an integer vector that is NOT in the lattice (x has an odd coefficient), halfway between the lattice points 0 and
    x b."""
    d = min(len(b), 12)
    for m in range(1, 1 << d):
        x = [(m >> i) & 1 for i in range(d)] + [0] * (len(b) - d)
        v = [sum(x[i] * b[i][j] for i in range(len(b))) for j in range(len(b[0]))]
        if all(u % 2 == 0 for u in v):
            return x, [u // 2 for u in v]
    return None


def targets(name):
    """[(kind, t)] integer targets around the lattice of a member: `near` — a lattice point with coefficients in
    [-8, 8] plus offsets in [-6, 6] (two of them); `far` — the same with coefficients around 2^30, where the entries
    still fit 63 bits; `half` — a lattice point plus half of a lattice vector with even entries, where the member has
    one: the target is then exactly halfway between two lattice points and every closest point has a twin."""
    key = ("targets", name)
    if key not in _exact:
        b = basis(name)
        d, n = len(b), len(b[0])
        rng = np.random.default_rng(sum(ord(c) for c in name))
        out = []

        def point(span):
            c = [int(v) for v in rng.integers(-span, span + 1, size=d)]
            return [sum(c[i] * b[i][j] for i in range(d)) for j in range(n)]

        for _ in range(2):
            out.append(("near", [p + int(o) for p, o in zip(point(8), rng.integers(-6, 7, size=n))]))
        far = [p + int(o) for p, o in zip(point(2**30), rng.integers(-6, 7, size=n))]
        if max(abs(v) for v in far) < 2**62:
            out.append(("far", far))
        ev = _even_combination(b)
        if ev is not None:
            out.append(("half", [p + h for p, h in zip(point(8), ev[1])]))
        _exact[key] = out
    return _exact[key]


# ---- what the CPU and the GPU tests ask of an answer -----------------------------------------------------------------
def _vector_of(b, x):
    return [sum(int(x[i]) * b[i][j] for i in range(len(b))) for j in range(len(b[0]))]


def check_shortest(name, sol, vec, norm, unit_rule=True):
    """What every shortest-vector answer is asked: the exact minimum, sol_coord one of the exact minimal vectors (up to
    sign: the set holds both), vec = sol_coord b in Python integers.  unit_rule: where a row of the basis is already
    minimal nothing is STRICTLY shorter, and the answer is the first such row (get_basis_min, svpcvp.cpp)."""
    ex, b = exact(name), basis(name)
    sol = tuple(int(v) for v in sol)
    assert int(norm) == ex["lam1"], (name, int(norm), ex["lam1"])
    assert sol in ex["minimal"], (name, sol)
    assert [int(v) for v in vec] == _vector_of(b, sol) and sum(int(v) ** 2 for v in vec) == int(norm)
    if unit_rule and ex["N0"] == ex["lam1"]:
        assert sol == tuple(int(i == ex["i0"]) for i in range(len(b))), (name, sol)


def check_pruned(name, pruning, sol, norm):
    """A pruned walk's answer, whatever its order: (a) it is a node of the exact pruned tree at the first radius
    N0 - 1 (the bounds only shrink), the 2^-30 margin allowed for; (b) the exact pruned tree at radius norm - 1 is
    empty — the walk ends with that radius and everything it cut before was cut at a larger one."""
    ex, b = exact(name), basis(name)
    import exact_lattice as X
    from fractions import Fraction
    de = ex["d_eff"]
    lev = [Fraction(float(v)) for v in pruning[:de]]
    sol = tuple(int(v) for v in sol)
    assert not any(sol[de:]) and sum(v * v for v in X.vector_of(b, sol)) == int(norm) <= ex["N0"]
    if int(norm) < ex["N0"]:
        pd = X.partial_distances(b[:de], sol[:de])
        R0 = (ex["N0"] - 1) * (1 + Fraction(1, 2**29))
        assert all(pd[k] <= lev[k] * R0 for k in range(de)), "the answer is outside the pruned tree"
    else:
        assert sol == tuple(int(i == ex["i0"]) for i in range(len(b)))
    assert X.short_exact(b, int(norm) - 1, rows=de, level=lev, max_nodes=NODE_CAP)[0] == [], "a shorter vector within the bounds"


# (the first three hold a shorter vector than their rows WITHIN these bounds: a pruned walk has something to find)
PRUNED = ["root_e8_s29_full_0", "root_e8_s20_x3_0", "root_e8_s10_x2_0", "knap_d20_b40", "knap_d12_b30", "steep_63"]


def pruning_of(name):
    import exact_enum as E
    return [float(v) for v in E.step_pruning(len(basis(name)), low=0.75)]


# ---- the mixed AUTO batch ---------------------------------------------------------------------------------------------
MIXED_FIRST, MIXED_COUNT = 1, 9


def mixed_batch():
    """([11][16][17] integers, roles): easy lattices (1000 on the diagonal, entries in [-3, 3] elsewhere: a tiny node
    estimate) and hard ones (knapsack, 40 bits: dense) interleaved, one with an entry of 2^62 (status -2) and one with
    two equal rows (update_gso fails: status 0); the solver tests call the sub-range [1, 10).  Once per process."""
    if "mixed" not in _exact:
        rng = np.random.default_rng(1617)
        roles = ["easy", "hard", "big", "easy", "hard", "equal", "easy", "hard", "easy", "hard", "easy"]
        bs, seed = [], 0
        for k, role in enumerate(roles):
            if role == "hard":
                bs.append(knapsack(16, 40, seed))
                seed += 1
                continue
            b = [[(1000 + 7 * i) * int(i == j) + int(rng.integers(-3, 4)) for j in range(17)] for i in range(16)]
            if role == "big":
                b[5] = [0] * 17
                b[5][3] = b[5][16] = 2**62
            if role == "equal":
                b[9] = list(b[4])
            bs.append(b)
        _exact["mixed"] = (bs, roles)
    return _exact["mixed"]
