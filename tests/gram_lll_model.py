"""Plain restatement of fplll's MatGSOGram<Z_NR<long>, FP_NR<double>>(g, u, u_inv_t, GSO_INT_GRAM) and of
LLLReduction<Z_NR<long>, FP_NR<double>>::lll() over it: Python integers wrapped to 64 bits for Z_NR<long>, Python
floats (IEEE doubles: every product, difference and quotient is one rounded operation, as FP_NR<double>'s) for the
floating-point side, one operation per reference operation, in the reference's order.

  lll.cpp:44-164, :166-224; gso_gram.cpp:25-400; gso_gram.h:153-262; gso_interface.cpp:26-53, :131-164;
  nr/matrix.cpp:65-93 (rotate_gram_left / _right), :127-134 (get_max_exp); nr/nr_Z_l.inl:30-48; nr/nr_FP_d.inl:44-53,
  :226-233.

Nothing here is tuned to the device: the matrix g is the reference's (only its lower triangle is kept up to date,
the upper one holds whatever the rotations leave there until symmetrize_g), move_row rotates g over the range the
reference rotates it, n_known_rows included.  `max_abs` records the largest |entry| ever written to g, BEFORE
wrapping: parity with the reference is promised while it stays below 2^63 (tests keep it below 2^62).
"""
import math

_M64 = (1 << 64) - 1

# statuses of fphip_gso_lll / fphip_gram_lll, and fplll's RedStatus (defs.h) they stand for
OK, GSO_FAILURE, BABAI_FAILURE, LLL_FAILURE = 1, 0, -1, -3
FROM_REF_STATUS = {0: OK, 2: GSO_FAILURE, 3: BABAI_FAILURE, 4: LLL_FAILURE}
LLL_VERBOSE, LLL_EARLY_RED, LLL_SIEGEL = 1, 2, 4


def wrap(x):
    x &= _M64
    return x - (1 << 64) if x >> 63 else x


def z_exponent(v):
    """Z_NR<long>::exponent()"""
    f, e = math.frexp(float(v))
    if v > (1 << 53) and abs(f) == 0.5:
        return abs(v).bit_length()
    return e


def f_exponent(x):
    """FP_NR<double>::exponent() = ilogb(x) + 1 (glibc: ilogb(0) = INT_MIN)"""
    if x == 0.0:
        return -(1 << 31) + 1
    return math.frexp(x)[1]


def rnd_we(b, expo_add):
    if f_exponent(b) + expo_add >= 53:
        return b
    return math.ldexp(float(round(math.ldexp(b, expo_add))), -expo_add)  # round(): to nearest, ties to even = rint


class BabaiFailure(Exception):
    pass


class MatGSOGram:
    def __init__(self, g, with_u=True):
        self.d = d = len(g)
        self.g = [[int(x) for x in row] for row in g]
        self.u = [[1 if i == j else 0 for j in range(d)] for i in range(d)] if with_u else None
        self.mu = [[0.0] * d for _ in range(d)]
        self.r = [[0.0] * d for _ in range(d)]
        self.valid = [0] * d
        self.n_known_rows = 0
        self.max_abs = max([abs(x) for row in self.g for x in row] + [0])

    # ---- g through sym_g (gso_interface.h:664-672)
    def sg(self, i, j):
        return self.g[i][j] if i >= j else self.g[j][i]

    def sg_set(self, i, j, v):
        a = abs(v)
        if a > self.max_abs:
            self.max_abs = a
        v = wrap(v)
        if i >= j:
            self.g[i][j] = v
        else:
            self.g[j][i] = v

    def gii_add(self, i, v):
        self.sg_set(i, i, self.g[i][i] + v)

    def get_gram(self, i, j):
        return float(self.g[i][j])  # f.set_z(g(i, j)): the nearest double

    def get_max_exp_of_b(self):
        m = 0
        for row in self.g:
            for x in row:
                m = max(m, z_exponent(x))
        return m // 2

    def b_row_is_zero(self, i):
        return self.g[i][i] == 0

    # ---- row operations (gso_gram.cpp:51-142)
    def _u_addmul(self, i, j, x):
        if self.u is not None:
            ui, uj = self.u[i], self.u[j]
            for k in range(self.d):
                ui[k] = wrap(ui[k] + uj[k] * x)

    def row_add(self, i, j):
        self._u_addmul(i, j, 1)
        t = wrap(self.sg(i, j) * 2)
        t = wrap(t + self.g[j][j])
        self.gii_add(i, t)
        for k in range(self.d):
            if k != i:
                self.sg_set(i, k, self.sg(i, k) + self.sg(j, k))

    def row_sub(self, i, j):
        self._u_addmul(i, j, -1)
        t = wrap(self.sg(i, j) * 2)
        t = wrap(self.g[j][j] - t)
        self.gii_add(i, t)
        for k in range(self.d):
            if k != i:
                self.sg_set(i, k, self.sg(i, k) - self.sg(j, k))

    def row_addmul_si(self, i, j, x):
        self._u_addmul(i, j, x)
        t = wrap(wrap(self.sg(i, j) * x) * 2)
        self.gii_add(i, t)
        t = wrap(wrap(self.g[j][j] * x) * x)
        self.gii_add(i, t)
        for k in range(self.d):
            if k == i:
                continue
            self.sg_set(i, k, self.sg(i, k) + wrap(self.sg(j, k) * x))

    def row_addmul_we(self, i, j, x, expo_add):
        expo = 0 if x == 0.0 else max(f_exponent(x) + expo_add - 63, 0)
        lx = int(math.ldexp(x, expo_add - expo))
        if expo != 0:
            raise NotImplementedError("multiplier beyond 63 bits (row_addmul_si_2exp): outside the parity range")
        if lx == 1:
            self.row_add(i, j)
        elif lx == -1:
            self.row_sub(i, j)
        elif lx != 0:
            self.row_addmul_si(i, j, lx)

    def row_op_end(self, first, last):
        for i in range(first, last):
            self.valid[i] = min(self.valid[i], 0)
        for i in range(last, self.n_known_rows):
            self.valid[i] = min(self.valid[i], first)

    # ---- nr/matrix.cpp:65-93 on the whole matrix, stale upper triangle included
    @staticmethod
    def _rotl(v, first, last):
        v[first:last + 1] = v[first + 1:last + 1] + [v[first]]

    @staticmethod
    def _rotr(v, first, last):
        v[first:last + 1] = [v[last]] + v[first:last]

    def rotate_gram_left(self, first, last, n_valid_rows):
        m = self.g
        m[first][first], m[first][last] = m[first][last], m[first][first]
        for i in range(first, last):
            m[i + 1][first], m[first][i] = m[first][i], m[i + 1][first]
        for i in range(first, n_valid_rows):
            self._rotl(m[i], first, min(last, i))
        self._rotl(m, first, last)

    def rotate_gram_right(self, first, last, n_valid_rows):
        m = self.g
        self._rotr(m, first, last)
        for i in range(first, n_valid_rows):
            self._rotr(m[i], first, min(last, i))
        for i in range(first, last):
            m[i + 1][first], m[first][i] = m[first][i], m[i + 1][first]
        m[first][first], m[first][last] = m[first][last], m[first][first]

    def move_row(self, old_r, new_r):
        d = self.d
        if new_r < old_r:
            for i in range(new_r, self.n_known_rows):
                self.valid[i] = min(self.valid[i], new_r)
            self._rotr(self.valid, new_r, old_r)
            self._rotr(self.mu, new_r, old_r)
            self._rotr(self.r, new_r, old_r)
            if self.u is not None:
                self._rotr(self.u, new_r, old_r)
            self.rotate_gram_right(new_r, old_r, d)
        elif new_r > old_r:
            for i in range(old_r, self.n_known_rows):
                self.valid[i] = min(self.valid[i], old_r)
            self._rotl(self.valid, old_r, new_r)
            self._rotl(self.mu, old_r, new_r)
            self._rotl(self.r, old_r, new_r)
            if self.u is not None:
                self._rotl(self.u, old_r, new_r)
            if old_r < self.n_known_rows - 1:
                self.rotate_gram_left(old_r, min(new_r, self.n_known_rows - 1), d)
            if new_r >= self.n_known_rows:
                if old_r < self.n_known_rows:
                    self.n_known_rows -= 1

    # ---- gso_interface.cpp:131-164
    def update_gso_row(self, i, last_j=None):
        if last_j is None:
            last_j = i
        if i >= self.n_known_rows:
            self.n_known_rows += 1  # discover_row(), gso_gram.cpp:25-39
            self.valid[i] = 0
        j = max(0, self.valid[i])
        ri, mui = self.r[i], self.mu[i]
        while j <= last_j:
            f = self.get_gram(i, j)
            muj = self.mu[j]
            for k in range(j):
                f = f - muj[k] * ri[k]
            ri[j] = f
            if i > j:
                rjj = self.r[j][j]
                if rjj == 0.0:
                    q = math.nan if (f == 0.0 or f != f) else math.copysign(math.inf, f) * math.copysign(1.0, rjj)
                else:
                    q = f / rjj
                mui[j] = q
                if not math.isfinite(q):
                    return False
            j += 1
        self.valid[i] = j
        return True

    def symmetrize_g(self):
        d = self.d
        self.g = [[self.sg(i, j) for j in range(d)] for i in range(d)]


def lll(g, delta=0.99, eta=0.51, flags=0, with_u=True):
    """LLLReduction(m, delta, eta, flags).lll() on a fresh MatGSOGram of g.  Returns a dict: g (after
    symmetrize_g), u, status (the device's convention), final_kappa, n_swaps, zeros, iterations, max_abs."""
    m = MatGSOGram(g, with_u)
    d = m.d
    siegel = bool(flags & LLL_SIEGEL)  # (LLL_EARLY_RED is switched off with enable_int_gram, lll.cpp:35)
    swap_threshold = delta - eta * eta if siegel else delta
    kappa_min, kappa_start, kappa_end = 0, 0, d
    res = {"final_kappa": 0, "n_swaps": 0, "zeros": 0, "iterations": 0}

    def babai(kappa):
        max_expo = None
        it = 0
        while True:
            if not m.update_gso_row(kappa, kappa - 1):
                return GSO_FAILURE
            mu_k = m.mu[kappa]
            if not any(abs(mu_k[j]) > eta for j in range(kappa)):
                return OK
            if it >= 2:
                new_max = max(f_exponent(mu_k[j]) for j in range(kappa))
                if max_expo is not None and new_max > max_expo - 5:
                    return BABAI_FAILURE
                max_expo = new_max
            babai_mu = mu_k[:kappa]
            for j in range(kappa - 1, -1, -1):
                x = rnd_we(babai_mu[j], 0)
                if x == 0.0:
                    continue
                muj = m.mu[j]
                for k in range(j):
                    babai_mu[k] = babai_mu[k] - x * muj[k]
                m.row_addmul_we(kappa, j, -x, 0)
            m.row_op_end(kappa, kappa + 1)
            it += 1

    zeros = 0
    while zeros < d and m.b_row_is_zero(0):
        m.move_row(kappa_min, kappa_end - 1 - zeros)
        zeros += 1
    status = None
    if zeros < d and not m.update_gso_row(kappa_start):
        status = GSO_FAILURE
        res["final_kappa"] = kappa_start
    kappa = kappa_start + 1
    n_swaps = 0
    it = 0
    if status is None:
        max_iter = int(d - 2 * d * (d + 1) * ((m.get_max_exp_of_b() + 3) / math.log(delta)))
        lt = [0.0] * (d + 1)
        while it < max_iter and kappa < kappa_end - zeros:
            rc = babai(kappa)
            if rc != OK:
                status = rc
                res["final_kappa"] = kappa
                break
            lt[0] = m.get_gram(kappa, kappa)
            mu_k, r_k = m.mu[kappa], m.r[kappa]
            for i in range(1, kappa + 1):
                lt[i] = lt[i - 1] - mu_k[i - 1] * r_k[i - 1]
            f = m.r[kappa - 1][kappa - 1] * swap_threshold
            if f > lt[kappa if siegel else kappa - 1]:
                n_swaps += 1
                old_k = kappa
                kappa -= 1
                while kappa > kappa_min:
                    f = m.r[kappa - 1][kappa - 1] * swap_threshold
                    if f < lt[kappa if siegel else kappa - 1]:
                        break
                    kappa -= 1
                if lt[kappa] > 0:
                    m.move_row(old_k, kappa)
                else:
                    zeros += 1
                    m.move_row(old_k, kappa_end - zeros)
                    kappa = old_k
                    it += 1
                    continue
            m.r[kappa][kappa] = lt[kappa]  # set_r(kappa, kappa, .)
            if m.valid[kappa] == kappa:
                m.valid[kappa] = kappa + 1
            kappa += 1
            it += 1
        if status is None:
            m.symmetrize_g()
            status = LLL_FAILURE if kappa < kappa_end - zeros else OK
    res.update(g=m.g, u=m.u, status=status, n_swaps=n_swaps, zeros=zeros, iterations=it, max_abs=m.max_abs)
    return res


def update_gso(g):
    """update_gso() of a fresh MatGSOGram of g: (mu, r, rows) — rows = the rows whose update_gso_row succeeded."""
    m = MatGSOGram(g, with_u=False)
    rows = 0
    while rows < m.d and m.update_gso_row(rows):
        rows += 1
    return m.mu, m.r, rows
