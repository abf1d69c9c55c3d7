"""Host-side mirror of fplll's MatHouseholder interface (fplll/householder.h) for a BATCH of
lattices on the GPU: ``refresh_R_bf(); update_R(); get_R(expo)``.  No arithmetic here."""
import ctypes

import numpy as np

from . import _lib


def _bind(lib):
    if getattr(lib, "_hh_bound", False):
        return
    vp = ctypes.c_void_p
    lib.fphip_hh_create.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(vp)]
    lib.fphip_hh_create.restype = ctypes.c_int
    lib.fphip_hh_destroy.argtypes = [vp]
    lib.fphip_hh_destroy.restype = None
    lib.fphip_hh_set_basis.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
    lib.fphip_hh_broadcast_basis.argtypes = [vp, ctypes.c_int]
    lib.fphip_hh_update_R.argtypes = [vp, vp]
    lib.fphip_hh_update_R_blocked.argtypes = [vp, vp]
    lib.fphip_hh_update_R_blocked.restype = ctypes.c_int
    lib.fphip_hh_hlll_ex.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                     ctypes.c_int, vp, vp]
    lib.fphip_hh_hlll_ex.restype = ctypes.c_int
    lib.fphip_hh_hlll_ladder.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                         vp, vp, vp]
    lib.fphip_hh_hlll_ladder.restype = ctypes.c_int
    lib.fphip_hh_get_R_lo.argtypes = [vp, ctypes.c_int, vp]
    lib.fphip_hh_get_R_lo.restype = ctypes.c_int
    lib.fphip_hh_get_R_plane.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
    lib.fphip_hh_get_R_plane.restype = ctypes.c_int
    lib.fphip_hh_get_basis.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
    lib.fphip_hh_hlll.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                  ctypes.c_double, vp, vp]
    lib.fphip_hh_get_R.argtypes = [vp, ctypes.c_int, vp]
    lib.fphip_hh_size_reduce.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
    lib.fphip_hh_size_reduce.restype = ctypes.c_int
    lib.fphip_hh_get_row_expo.argtypes = [vp, ctypes.c_int, vp]
    lib.fphip_hh_last_kernel_ms.argtypes = [vp]
    lib.fphip_hh_last_kernel_ms.restype = ctypes.c_double
    lib._hh_bound = True


class MatHouseholderBatch:
    def __init__(self, ctx, batch, d, n, row_expo=False):
        self.ctx, self.lib = ctx, ctx.lib
        ctx.adopt(self)
        _bind(self.lib)
        self.batch, self.d, self.n = batch, d, n
        self.h = ctypes.c_void_p()
        rc = self.lib.fphip_hh_create(ctx.handle, batch, d, n, 1 if row_expo else 0,
                                      ctypes.byref(self.h))
        if rc == _lib.FPHIP_UNSUPPORTED:
            raise NotImplementedError("d, n > 256 are not handled on the device")
        if rc != _lib.FPHIP_OK:
            raise _lib.HipError("fphip_hh_create: " + ctx.last_error())

    def _chk(self, rc, what):
        if rc != _lib.FPHIP_OK:
            raise _lib.HipError("%s: %s" % (what, self.ctx.last_error()))

    def set_basis(self, b, first=0):
        b = np.ascontiguousarray(b, dtype=np.int64)
        if b.ndim == 2:
            b = b[None]
        assert b.shape[1:] == (self.d, self.n)
        self._chk(self.lib.fphip_hh_set_basis(self.h, first, b.shape[0],
                                              b.ctypes.data_as(ctypes.c_void_p)), "set_basis")

    def broadcast_basis(self, src=0):
        self._chk(self.lib.fphip_hh_broadcast_basis(self.h, src), "broadcast_basis")

    def enable_transform(self, u=None):
        """MatHouseholder(b, u, u_inv, flags) with a non-empty u: track the transformation matrix on the device —
        u [batch][d][d] int64, or None for the identity.  hlll() at every precision, hlll_ladder() and size_reduce()
        then apply every row operation to u as well (householder.cpp:372-398, 456-559); update_R() does not touch b.
        set_basis() keeps u, broadcast_basis() copies it with b, a second call resets it.  Needs d <= n."""
        fn = self.lib.fphip_hh_enable_transform
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.int64)
            assert u.shape == (self.batch, self.d, self.d)
        rc = fn(self.h, None if u is None else u.ctypes.data_as(ctypes.c_void_p))
        if rc == _lib.FPHIP_UNSUPPORTED:
            raise NotImplementedError("enable_transform: " + self.ctx.last_error())
        self._chk(rc, "enable_transform")

    def get_transform(self, first=0, count=None):
        count = self.batch - first if count is None else count
        u = np.empty((count, self.d, self.d), dtype=np.int64)
        fn = self.lib.fphip_hh_get_transform
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        self._chk(fn(self.h, first, count, u.ctypes.data_as(ctypes.c_void_p)), "get_transform")
        return u

    def get_inverse_transform_t(self, first=0, count=None):
        """The inverse transpose of the u the device tracks — an integer matrix, u being unimodular.  It is the
        reference's u_inv_t (MatHouseholder(b, u, u_inv, ...) with enable_inverse_transform, householder.cpp:456-559:
        every row operation b_i += x b_j is mirrored as u_inv_t_j -= x u_inv_t_i) ONLY for a u that started at the
        identity.  DERIVED ON THE HOST (exact integer elimination, `gso.inverse_transpose`); the device keeps no
        u_inv_t of its own.  [count][d][d] Python-int object arrays (entries may leave int64)."""
        from .gso import inverse_transpose
        u = self.get_transform(first, count)
        return np.stack([inverse_transpose(m) for m in u])

    def update_R(self, blocked=False):
        """refresh_R_bf() + update_R() for every lattice.  blocked=True: the opt-in MFMA compact-WY
        mode (same R to rounding — 1e-9 on mu / r —, not bit for bit)."""
        st = np.zeros(self.batch, dtype=np.int32)
        fn = self.lib.fphip_hh_update_R_blocked if blocked else self.lib.fphip_hh_update_R
        self._chk(fn(self.h, st.ctypes.data_as(ctypes.c_void_p)), "update_R")
        return st

    def size_reduce(self, kappa, size_reduction_end=None, size_reduction_start=0):
        """MatHouseholder::size_reduce(k, size_reduction_end, size_reduction_start) (householder.cpp:402-451) on every
        lattice, on the state update_R() left.  Returns (reduced[batch], status[batch])."""
        end = kappa if size_reduction_end is None else size_reduction_end
        red = np.zeros(self.batch, dtype=np.int32)
        st = np.zeros(self.batch, dtype=np.int32)
        self._chk(self.lib.fphip_hh_size_reduce(self.h, int(kappa), int(end), int(size_reduction_start),
                                                red.ctypes.data_as(ctypes.c_void_p),
                                                st.ctypes.data_as(ctypes.c_void_p)), "size_reduce")
        return red, st

    def get_basis(self, first=0, count=1):
        b = np.empty((count, self.d, self.n), dtype=np.int64)
        self._chk(self.lib.fphip_hh_get_basis(self.h, first, count,
                                              b.ctypes.data_as(ctypes.c_void_p)), "get_basis")
        return b

    def hlll(self, delta=0.99, eta=0.51, theta=0.001, c=0.1, precision=None):
        """HLLLReduction::hlll() on every lattice (fplll/hlll.cpp:26-169).
        precision None: the exact-order double kernel (bit-identical decisions); 106: double-double
        arithmetic (FP_NR<dd_real>'s stand-in), 212: quad-double (FP_NR<qd_real>'s), 53: double — all with tree sums
        (hlll_x.hip).
        Returns (status[batch], info[batch][2] = swaps, iterations)."""
        st = np.zeros(self.batch, dtype=np.int32)
        info = np.zeros((self.batch, 2), dtype=np.int32)
        if precision is None:
            self._chk(self.lib.fphip_hh_hlll(self.h, delta, eta, theta, c,
                                             st.ctypes.data_as(ctypes.c_void_p),
                                             info.ctypes.data_as(ctypes.c_void_p)), "hlll")
        else:
            self._chk(self.lib.fphip_hh_hlll_ex(self.h, delta, eta, theta, c, int(precision),
                                                st.ctypes.data_as(ctypes.c_void_p),
                                                info.ctypes.data_as(ctypes.c_void_p)), "hlll_ex")
        return st, info

    def hlll_ladder(self, delta=0.99, eta=0.51, theta=0.001, c=0.1):
        """The wrapper's precision ladder on the device: double for the batch, double-double for the
        lattices that raise a precision alarm, quad-double for those it gives up on (wrapper.cpp:478-529, 630-710).
        Returns (status, info, stage[batch] in {53, 106, 212})."""
        st = np.zeros(self.batch, dtype=np.int32)
        info = np.zeros((self.batch, 2), dtype=np.int32)
        stage = np.zeros(self.batch, dtype=np.int32)
        self._chk(self.lib.fphip_hh_hlll_ladder(self.h, delta, eta, theta, c, st.ctypes.data_as(ctypes.c_void_p),
                                                info.ctypes.data_as(ctypes.c_void_p),
                                                stage.ctypes.data_as(ctypes.c_void_p)), "hlll_ladder")
        return st, info, stage

    def get_R_lo(self, lattice=0):
        """low plane of R after hlll(precision=106)"""
        R = np.empty((self.d, self.n))
        self._chk(self.lib.fphip_hh_get_R_lo(self.h, lattice, R.ctypes.data_as(ctypes.c_void_p)), "get_R_lo")
        return R

    def get_R_plane(self, lattice=0, plane=0):
        """component plane 0..3 of R after hlll(precision=...): R is the sum of the planes (one at 53 bits, two at
        106, four at 212; the others read as zeros) times 2^row_expo"""
        R = np.empty((self.d, self.n))
        self._chk(self.lib.fphip_hh_get_R_plane(self.h, lattice, int(plane), R.ctypes.data_as(ctypes.c_void_p)),
                  "get_R_plane")
        return R

    def get_R(self, lattice=0):
        R = np.empty((self.d, self.n))
        self._chk(self.lib.fphip_hh_get_R(self.h, lattice, R.ctypes.data_as(ctypes.c_void_p)), "get_R")
        e = np.empty(self.d, dtype=np.int64)
        self._chk(self.lib.fphip_hh_get_row_expo(self.h, lattice, e.ctypes.data_as(ctypes.c_void_p)),
                  "get_row_expo")
        return R, e

    @property
    def last_kernel_ms(self):
        return float(self.lib.fphip_hh_last_kernel_ms(self.h))

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "handle", None):  # (a closed context has released everything)
                self.lib.fphip_hh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
