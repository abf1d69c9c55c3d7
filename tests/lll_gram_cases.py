"""Shared by tests/test_lll_gram_cpu.py and tests/test_lll_gram_gpu.py: the fixtures tests/golden/lllgram_*.json(.gz)
(recorded from the reference by tests/native/lll_gram_ref_driver.cpp, tests/golden/make_lll_gram_fixtures.sh), the
model's run of each (computed once per process), and the seeded random forms no fixture holds."""
import glob
import gzip
import hashlib
import json
import os

import numpy as np

import conftest as C
import gram_lll_model as M


def wide_basis(d):
    """The basis behind the width-class fixtures w<d>, from integer arithmetic alone (a 64-bit linear congruential
    generator, so the fixture need not store it): a perturbed multiple of the identity — reduced but for rounding —
    with three multiples in [-3, 3] of earlier ORIGINAL rows added to every row (the recipe of gso._unreduced_copy
    without its compounding, which reaches 2^16 at 256 rows: forms the reference's double precision gives up on) and
    one pair of neighbours per 64 rows exchanged, so that the swap test and the insertion index run in every chunk."""
    state = [d * 2654435761 + 12345]

    def rnd(n):
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
        return (state[0] >> 33) % n
    b0 = np.array([[(24 if i == j else 0) + rnd(5) - 2 for j in range(d)] for i in range(d)], dtype=np.int64)
    b = b0.copy()
    for i in range(1, d):
        for _ in range(3):
            j = rnd(i)
            b[i] += (rnd(7) - 3) * b0[j]
    for p in range(40, d - 1, 64):
        b[[p, p + 1]] = b[[p + 1, p]]
    return b


def digest_int(m):
    """SHA-256 of an integer matrix as little-endian int64, row by row."""
    return hashlib.sha256(np.ascontiguousarray(m, dtype="<i8").tobytes()).hexdigest()


def digest_tri(full, rows, strict):
    """SHA-256 of the first `rows` rows of a lower triangle (j < i, or j <= i) as little-endian doubles: equal
    digests are equal bits."""
    h = hashlib.sha256()
    for i in range(rows):
        h.update(np.array(full[i][:i if strict else i + 1], dtype="<f8").tobytes())
    return h.hexdigest()


def compact(f):
    """What a width-class fixture stores of the driver's record: u and the counters as they are; of G_in, G_out, mu
    and r (two million numbers over the seven forms) the SHA-256 of their bits, and the diagonal of r.  A is
    wide_basis(d).  The recording script makes this only after checking u G_in u^T == G_out on the full record."""
    d = f["d"]
    out = {k: f[k] for k in ("name", "d", "delta", "eta", "flags", "status", "final_kappa", "n_swaps", "zeros",
                             "gso_rows", "ref_ms", "u")}
    mu = [[float.fromhex(x) for x in row] for row in f["mu"]]
    r = [[float.fromhex(x) for x in row] for row in f["r"]]
    out["r_diag"] = [f["r"][i][i] for i in range(f["gso_rows"])]
    out["sha256"] = {"G_in": digest_int(f["G_in"]), "G_out": digest_int(f["G_out"]),
                     "mu": digest_tri(mu, f["gso_rows"], True), "r": digest_tri(r, f["gso_rows"], False)}
    assert f["A"] == wide_basis(d).tolist()
    return out


def _load(path):
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as fh:
        f = json.load(fh)
    f["delta"] = float.fromhex(f["delta"])
    f["eta"] = float.fromhex(f["eta"])
    if "sha256" in f:
        # a compact record: the basis from its recipe, the forms from it and u — g_out = (u A)(u A)^T is the
        # congruence u G_in u^T, and its digest is compared with the one of the reference's own g_out
        a = wide_basis(f["d"])
        f["A"] = a.tolist()
        f["G_in"] = a.dot(a.T).tolist()
        ua = np.array(f["u"], dtype=np.int64).dot(a)
        f["G_out"] = ua.dot(ua.T).tolist()
        f["r_diag"] = [float.fromhex(x) for x in f["r_diag"]]
        return f
    f["mu"] = [[float.fromhex(x) for x in row] for row in f["mu"]]
    f["r"] = [[float.fromhex(x) for x in row] for row in f["r"]]
    return f


def same_gso(f, mu, r):
    """mu / r ([d][d], of the model or the device) against the fixture's, bit for bit, on its gso_rows rows"""
    rows = f["gso_rows"]
    if "sha256" in f:
        return (digest_tri(mu, rows, True) == f["sha256"]["mu"] and digest_tri(r, rows, False) == f["sha256"]["r"]
                and [float(r[i][i]) for i in range(rows)] == f["r_diag"])
    return tri_equal(f["mu"][:rows], mu, strict=True) and tri_equal(f["r"][:rows], r, strict=False)


def fixture_names():
    names = []
    for p in sorted(glob.glob(os.path.join(C.GOLDEN, "lllgram_*.json*"))):
        names.append(os.path.basename(p).split(".json")[0][len("lllgram_"):])
    return names


_fix, _model = {}, {}


def fixture(name):
    if name not in _fix:
        p = os.path.join(C.GOLDEN, "lllgram_%s.json" % name)
        _fix[name] = _load(p if os.path.exists(p) else p + ".gz")
    return _fix[name]


def model_run(name):
    """The model's lll() of the fixture's form, once per process."""
    if name not in _model:
        f = fixture(name)
        _model[name] = M.lll(f["G_in"], f["delta"], f["eta"], f["flags"])
    return _model[name]


def model_gso(name):
    """update_gso() of the model's reduced form, once per process: (mu, r, rows)."""
    if ("gso", name) not in _model:
        _model[("gso", name)] = M.update_gso(model_run(name)["g"])
    return _model[("gso", name)]


def tri_equal(rows, full, strict):
    """rows: the fixture's / model's triangle, row i holding j < i (strict) or j <= i; full: [d][d]; bit for bit."""
    for i, row in enumerate(rows):
        n = i if strict else i + 1
        a = np.array(row[:n], dtype=np.float64)
        b = np.array(full[i][:n], dtype=np.float64)
        if a.tobytes() != b.tobytes():
            return False
    return True


# ---- seeded random forms that no fixture holds
def random_forms(count, d, bits, seed):
    """`count` DISTINCT forms A A^T of random d x d integer matrices with entries of `bits` bits."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        a = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), size=(d, d)).astype(object)
        out.append(np.array(a.dot(a.T), dtype=np.int64))
    return np.stack(out)


def lightly_unreduced_forms(count, d, seed):
    """`count` distinct well-conditioned forms that need a size reduction and a few swaps: A A^T for a perturbed
    multiple of the identity with a few multiples of earlier rows added to every row and one pair of neighbours per
    64 rows exchanged (the recipe of the w* fixtures, without the reduction in between)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        b0 = 24 * np.eye(d, dtype=np.int64) + rng.integers(-2, 3, size=(d, d))
        b = b0.copy()
        for i in range(1, d):
            for _ in range(3):
                b[i] += int(rng.integers(-3, 4)) * b0[int(rng.integers(0, i))]
        for p in range(40, d - 1, 64):
            b[[p, p + 1]] = b[[p + 1, p]]
        out.append(b.dot(b.T))
    return np.stack(out)
