"""Lattices given as quadratic forms: a batch of integer Gram matrices on the GPU.

``MatGSOGramBatch`` mirrors fplll's ``MatGSOGram<Z_NR<long>, FP_NR<double>>(g, u, u_inv_t, GSO_INT_GRAM)``
(fplll/gso_gram.h) together with ``LLLReduction::lll`` over it; every number is computed by the HIP kernels of
csrc/lll_gram.hip behind the ``fphip_gram_*`` entry points of include/fplll_hip.h.  There is no integer basis: the
results are the reduced form and the transformation u with g_out = u g_in u^T.
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
