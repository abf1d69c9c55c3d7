"""Lattices given as quadratic forms: a batch of integer Gram matrices on the GPU.

``MatGSOGramBatch`` mirrors fplll's ``MatGSOGram<Z_NR<long>, FP_NR<double>>(g, u, u_inv_t, GSO_INT_GRAM)``
(fplll/gso_gram.h) together with ``LLLReduction::lll`` over it; every number is computed by the HIP kernels of
csrc/lll_gram.hip behind the ``fphip_gram_*`` entry points of include/fplll_hip.h.  There is no integer basis: the
results are the reduced form and the transformation u with g_out = u g_in u^T.

``MatGSOGramBatch.shortest_vectors`` and the module functions ``shortest_vectors_gram`` / ``shortest_vector_gram`` are
the reference's ``shortest_vectors(MatGSOGram, ...)`` / ``shortest_vector(MatGSOGram, ...)``: the minimum of a positive
definite form and its N shortest vectors, decided on exact integers x G x^T (csrc/svp_gram.hip).
"""
import ctypes

import numpy as np

from . import _lib
from .gso import LLL_DEF_DELTA, LLL_DEF_ETA, is_lll_reduced

LLL_VERBOSE, LLL_EARLY_RED, LLL_SIEGEL = 1, 2, 4  # fplll/defs.h:222-227


def _bind(lib):
    if getattr(lib, "_gram_bound", False):
        return
    vp = ctypes.c_void_p
    lib.fphip_gram_create.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    lib.fphip_gram_create.restype = ctypes.c_int
    lib.fphip_gram_destroy.argtypes = [vp]
    lib.fphip_gram_destroy.restype = None
    for name in ("fphip_gram_set", "fphip_gram_broadcast", "fphip_gram_get", "fphip_gram_get_mu", "fphip_gram_get_r",
                 "fphip_gram_get_transform", "fphip_gram_update"):
        getattr(lib, name).argtypes = [vp, vp]
        getattr(lib, name).restype = ctypes.c_int
    lib.fphip_gram_enable_transform.argtypes = [vp]
    lib.fphip_gram_enable_transform.restype = ctypes.c_int
    lib.fphip_gram_lll.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, vp, vp]
    lib.fphip_gram_lll.restype = ctypes.c_int
    lib.fphip_gram_last_kernel_ms.argtypes = [vp]
    lib.fphip_gram_last_kernel_ms.restype = ctypes.c_double
    lib._gram_bound = True


class MatGSOGramBatch:
    """`batch` independent d x d integer quadratic forms, state resident in HBM.  g: [batch][d][d] or one [d][d]."""

    def __init__(self, ctx, g):
        g = np.ascontiguousarray(g, dtype=np.int64)
        if g.ndim == 2:
            g = g[None]
        assert g.ndim == 3 and g.shape[1] == g.shape[2], g.shape
        self.ctx = ctx
        ctx.adopt(self)
        self.lib = ctx.lib
        _bind(self.lib)
        self.batch, self.d = g.shape[0], g.shape[1]
        self.h = ctypes.c_void_p()
        self.with_u = False
        rc = self.lib.fphip_gram_create(ctx.handle, self.batch, self.d, ctypes.byref(self.h))
        if rc == _lib.FPHIP_UNSUPPORTED:
            self.h = None
            raise NotImplementedError("d > 256 is not handled on the device")
        if rc != _lib.FPHIP_OK:
            self.h = None
            raise _lib.HipError("fphip_gram_create: " + ctx.last_error())
        self.set_gram(g)

    def _chk(self, rc, what):
        if rc != _lib.FPHIP_OK:
            raise _lib.HipError("%s: %s" % (what, self.ctx.last_error()))

    def set_gram(self, g):
        """Upload [batch][d][d]; a form that is not symmetric is refused (HipError), nothing is uploaded then."""
        g = np.ascontiguousarray(g, dtype=np.int64)
        if g.ndim == 2:
            g = g[None]
        assert g.shape == (self.batch, self.d, self.d), g.shape
        self._chk(self.lib.fphip_gram_set(self.h, g.ctypes.data_as(ctypes.c_void_p)), "set_gram")

    def broadcast(self, g):
        """One form [d][d] into every entry of the batch (device-side copies)."""
        g = np.ascontiguousarray(g, dtype=np.int64)
        assert g.shape == (self.d, self.d), g.shape
        self._chk(self.lib.fphip_gram_broadcast(self.h, g.ctypes.data_as(ctypes.c_void_p)), "broadcast")

    def gram(self):
        g = np.empty((self.batch, self.d, self.d), dtype=np.int64)
        self._chk(self.lib.fphip_gram_get(self.h, g.ctypes.data_as(ctypes.c_void_p)), "gram")
        return g

    def update(self):
        """update_gso() of every form; returns status[batch] (1, or 0 where a mu is not finite)."""
        st = np.zeros(self.batch, dtype=np.int32)
        self._chk(self.lib.fphip_gram_update(self.h, st.ctypes.data_as(ctypes.c_void_p)), "update")
        return st

    def _plane(self, fn, what):
        out = np.empty((self.batch, self.d, self.d), dtype=np.float64)
        self._chk(fn(self.h, out.ctypes.data_as(ctypes.c_void_p)), what)
        return out

    @property
    def mu(self):
        """[batch][d][d]: mu(i, j) for j < i, 0 elsewhere (of the last update() / lll())."""
        return self._plane(self.lib.fphip_gram_get_mu, "mu")

    @property
    def r(self):
        """[batch][d][d]: r(i, j) for j <= i, 0 elsewhere."""
        return self._plane(self.lib.fphip_gram_get_r, "r")

    def enable_transform(self):
        """Track u: every lll() starts it as the identity, get_transform() returns it afterwards."""
        self._chk(self.lib.fphip_gram_enable_transform(self.h), "enable_transform")
        self.with_u = True

    def get_transform(self):
        u = np.empty((self.batch, self.d, self.d), dtype=np.int64)
        self._chk(self.lib.fphip_gram_get_transform(self.h, u.ctypes.data_as(ctypes.c_void_p)), "get_transform")
        return u

    def lll(self, delta=LLL_DEF_DELTA, eta=LLL_DEF_ETA, flags=0):
        """LLLReduction(m, delta, eta, flags).lll() on every form.  Returns (status[batch], info[batch][4]):
        1 RED_SUCCESS, 0 RED_GSO_FAILURE, -1 RED_BABAI_FAILURE, -2 multiplier beyond 63 bits, -3 RED_LLL_FAILURE;
        info = final_kappa, n_swaps, zeros, loop iterations."""
        st = np.zeros(self.batch, dtype=np.int32)
        info = np.zeros((self.batch, 4), dtype=np.int32)
        self._chk(self.lib.fphip_gram_lll(self.h, float(delta), float(eta), int(flags),
                                          st.ctypes.data_as(ctypes.c_void_p), info.ctypes.data_as(ctypes.c_void_p)),
                  "lll")
        return st, info

    def is_lll_reduced(self, form=0, delta=LLL_DEF_DELTA, eta=LLL_DEF_ETA):
        """is_lll_reduced<ZT, double> (lll.cpp:226-258) on mu / r of the last update() / lll(); no row exponents."""
        return is_lll_reduced(self.mu[form], self.r[form], np.zeros(self.d, dtype=np.int64), delta, eta)

    def shortest_vectors(self, max_sols, bound_sq=None, pruning=None, route="auto", first=0, count=None, ectx=None,
                         method=0, flags=0):
        """fphip_gram_shortest_vectors: the ``max_sols`` (1 .. 64) shortest non-zero vectors, one of each pair +-x, of
        the forms [first, first + count) of the batch (LLL-reduced forms), decided on the exact integers x G x^T — the
        reference's shortest_vectors(MatGSOGram, ..., max_sols).  ``bound_sq``: None (the default bound: the smallest
        diagonal entry), one integer for every form, or [count] integers (0 = the default for that form); only vectors
        with norm <= the bound are kept.  ``route``: "wave" (one wavefront per form, d <= 64, the first max_sols vectors
        in (norm, depth-first discovery) order, deterministic), "enum" (one enumerator call per form; which of several
        vectors tied at the cut are kept is unspecified, the norms are not) or "auto" (the limit of the basis solver,
        FPHIP_SVP_WAVE_MAX_NODES, not retuned for forms).  Returns (found int32 [count], sol_coord int64
        [count][max_sols][d] — coefficients in the variables of the form as it stands on the device —, norm int64
        [count][max_sols] sorted, entries beyond found zero, nodes uint64 [count], status int32 [count]: 1, 0 = update
        failed or the form is not positive definite, -2 = a candidate beyond 63 bits).  With ``pruning`` found may be 0
        while status stays 1."""
        K = int(max_sols)
        if K != max_sols or K < 1 or K > 64:
            raise ValueError("shortest_vectors: max_sols is an integer in 1 .. 64, got %r" % (max_sols,))
        if route not in _lib.SVP_ROUTES:
            raise ValueError("shortest_vectors: route is one of %s, got %r" % (", ".join(sorted(_lib.SVP_ROUTES)), route))
        count = self.batch - first if count is None else int(count)
        if first < 0 or count < 1 or first + count > self.batch:
            raise ValueError("shortest_vectors: forms [%d, %d) outside the batch of %d" % (first, first + count, self.batch))
        bnd = None
        if bound_sq is not None:
            bnd = np.asarray(bound_sq)
            if bnd.ndim == 0:
                bnd = np.full(count, bnd)
            if bnd.shape != (count,) or any(int(v) != v or v < 0 or v >= 2**63 for v in bnd.tolist()):
                raise ValueError("shortest_vectors: bound_sq is None, a non-negative integer or [%d] of them, got %r" % (count, bound_sq))
            bnd = np.ascontiguousarray([int(v) for v in bnd.tolist()], dtype=np.int64)
        pr = None
        if pruning is not None:
            pr = np.ascontiguousarray(pruning, dtype=np.float64)
            if pr.shape != (self.d,):
                raise ValueError("shortest_vectors: pruning is [%d], got shape %r" % (self.d, pr.shape))
        found = np.zeros(count, dtype=np.int32)
        sol = np.zeros((count, K, self.d), dtype=np.int64)
        norm = np.zeros((count, K), dtype=np.int64)
        nodes = np.zeros(count, dtype=np.uint64)
        st = np.zeros(count, dtype=np.int32)
        fn = _lib.bind_gram_shortest_vectors(self.lib)
        rc = fn(self.h, None if ectx is None else ectx.handle, first, count, K,
                None if bnd is None else bnd.ctypes.data_as(ctypes.c_void_p), method, flags,
                None if pr is None else pr.ctypes.data_as(ctypes.c_void_p), _lib.SVP_ROUTES[route],
                *(a.ctypes.data_as(ctypes.c_void_p) for a in (found, sol, norm, nodes, st)))
        if rc == _lib.FPHIP_UNSUPPORTED:
            from .enumeration import Unsupported
            raise Unsupported("shortest_vectors declined by the device layer (d=%d): %s" % (self.d, self.ctx.last_error()))
        self._chk(rc, "shortest_vectors")
        return found, sol, norm, nodes, st

    @property
    def last_kernel_ms(self):
        return float(self.lib.fphip_gram_last_kernel_ms(self.h))

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "handle", None):  # (a closed context has released everything)
                self.lib.fphip_gram_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lll_reduction_gram(ctx, g, with_u=True, delta=LLL_DEF_DELTA, eta=LLL_DEF_ETA, flags=0):
    """LLL-reduce one quadratic form [d][d] or a batch [batch][d][d] on the device.  Returns (g_out, u, status): the
    reduced form(s), the transformation(s) with g_out = u g u^T (None without with_u), the status (an int for one
    form, an array for a batch)."""
    g = np.asarray(g, dtype=np.int64)
    single = g.ndim == 2
    m = MatGSOGramBatch(ctx, g)
    try:
        if with_u:
            m.enable_transform()
        st, _ = m.lll(delta, eta, flags)
        out = m.gram()
        u = m.get_transform() if with_u else None
    finally:
        m.close()
    if single:
        return out[0], (u[0] if with_u else None), int(st[0])
    return out, u, st


def sqnorm_coordinates(g, x):
    """x G x^T in Python integers: the reference's MatGSOGram::sqnorm_coordinates."""
    g = [[int(v) for v in row] for row in np.asarray(g, dtype=object).tolist()]
    x = [int(v) for v in np.asarray(x, dtype=object).reshape(-1).tolist()]
    if len(g) != len(x) or any(len(row) != len(x) for row in g):
        raise ValueError("sqnorm_coordinates: g is [d][d] and x [d], got %d rows and %d coefficients" % (len(g), len(x)))
    return sum(x[j] * sum(x[i] * g[i][j] for i in range(len(x)) if x[i]) for j in range(len(x)) if x[j])


def shortest_vectors_gram(ctx, g, max_sols, bound_sq=None, reduce=True, pruning=None, route="auto", ectx=None):
    """The ``max_sols`` (1 .. 64) shortest non-zero vectors, one of each pair +-x, of one quadratic form ``g`` (int64
    [d][d]) or of every form of a batch ([B][d][d]): the reference's shortest_vectors(MatGSOGram, ..., max_sols).
    ``bound_sq``: None (the smallest diagonal entry of the reduced form: at least one vector is found), one non-negative
    integer, or [B] of them (0 = the default).  ``reduce=True`` runs the batched Gram LLL with u first (the enumeration
    expects a reduced form) and returns ``sol_coord u`` in exact Python integers: coefficients in the CALLER's
    variables, sqnorm_coordinates(g, sol) == norm.  ``pruning`` / ``route`` as MatGSOGramBatch.shortest_vectors.
    Returns ``(found, sol_coord [max_sols][d], norm int64 [max_sols])`` for one form and ``(found int32 [B], sol_coord
    [B][max_sols][d], norm [B][max_sols])`` for a batch, sorted by norm, entries beyond found zero.  Raises ``HipError``
    naming the form where a status is not RED_SUCCESS."""
    ga = np.ascontiguousarray(g, dtype=np.int64)
    single = ga.ndim == 2
    if single:
        ga = ga[None]
    if ga.ndim != 3 or ga.shape[0] < 1 or ga.shape[1] < 1 or ga.shape[1] != ga.shape[2]:
        raise ValueError("shortest_vectors_gram: g is [d][d] or [B][d][d], got shape %r" % (np.shape(g),))
    if int(max_sols) != max_sols or not 1 <= max_sols <= 64:
        raise ValueError("shortest_vectors_gram: max_sols is an integer in 1 .. 64, got %r" % (max_sols,))
    if route not in _lib.SVP_ROUTES:
        raise ValueError("shortest_vectors_gram: route is one of %s, got %r" % (", ".join(sorted(_lib.SVP_ROUTES)), route))
    if pruning is not None and np.shape(pruning) != (ga.shape[1],):
        raise ValueError("shortest_vectors_gram: pruning is [%d], got shape %r" % (ga.shape[1], np.shape(pruning)))
    if bound_sq is not None:
        bq = np.asarray(bound_sq)
        if bq.shape not in ((), (ga.shape[0],)) or any(int(v) != v or v < 0 for v in bq.reshape(-1).tolist()):
            raise ValueError("shortest_vectors_gram: bound_sq is None, a non-negative integer or [%d] of them, got %r" % (ga.shape[0], bound_sq))
    m = MatGSOGramBatch(ctx, ga)
    try:
        u = None
        if reduce:
            m.enable_transform()
            status, _ = m.lll()
            for k, s in enumerate(status):
                if s != 1:
                    raise _lib.HipError("shortest_vectors_gram: lll of form %d ended with status %d" % (k, s))
            u = m.get_transform()
        found, sol, norm, _, status = m.shortest_vectors(int(max_sols), bound_sq=bound_sq, pruning=pruning, route=route, ectx=ectx)
    finally:
        m.close()
    for k, s in enumerate(status):
        if s != 1:
            raise _lib.HipError("shortest_vectors_gram: form %d ended with status %d (%s)" % (
                k, s, "a norm beyond 63 bits" if s == -2 else "update failed or the form is not positive definite"))
    if u is not None:  # x_in = sol u: the coefficients in the caller's variables, exact
        sol = np.stack([sol[k].astype(object).dot(u[k].astype(object)) for k in range(len(sol))])
    if single:
        return int(found[0]), sol[0], norm[0]
    return found, sol, norm


def shortest_vector_gram(ctx, g, reduce=True, pruning=None, route="auto", ectx=None):
    """A shortest non-zero vector of one form (``(sol_coord [d], norm)``) or of every form of a batch (``(sol_coord
    [B][d], norm int64 [B])``): the reference's shortest_vector(MatGSOGram, sol_coord, SVPM_FAST).  Arguments as
    ``shortest_vectors_gram`` with max_sols = 1.  A pruned walk that finds nothing raises ``HipError``."""
    single = np.ndim(g) == 2
    found, sol, norm = shortest_vectors_gram(ctx, g, 1, reduce=reduce, pruning=pruning, route=route, ectx=ectx)
    for k, f in enumerate([found] if single else found):
        if f != 1:
            raise _lib.HipError("shortest_vector_gram: form %d: nothing found within the pruned bounds" % k)
    if single:
        return sol[0], int(norm[0])
    return sol[:, 0], norm[:, 0]
