"""Host-side mirror of the reference's closest-vector solver (fplll/svpcvp.cpp:532-659, ``closest_vector``).

Everything is computed on the GPU behind ``fphip_closest_vector`` (include/fplll_hip.h): update_gso, the target
preparation kernel (Gram-Schmidt coordinates, the Babai loop), one closest-vector enumeration per target; nothing here
solves anything on the CPU.  The batched form is the workload the device is for: many targets against one reduced
basis.  ``route="wave"`` (``fphip_closest_vector_ex``) solves that batch in ONE launch, one wavefront per
target, for bases of at most 64 rows; ``route="auto"`` starts there and finishes the hard targets by enumerations;
the default, ``"enum"``, is the one-enumeration-per-target path.
"""
import numpy as np

from . import _lib
from .gso import MatGSOBatch, lll_reduction

CVPM_FAST = 0
CVPM_PROVED = 2  # declined (Unsupported): the max_indices reset path of the enumeration is not offered
RED_SUCCESS = 1


def closest_vectors(ctx, b, targets, reduce=False, method=CVPM_FAST, ectx=None, with_dist=False, route="enum",
                    max_nodes=0):
    """closest_vector(b, target, sol_coord, method) for every row of ``targets`` (int64 [T][n]) against the basis
    ``b`` (int64 [d][n], d <= n), which is expected LLL-reduced as the reference expects.  ``reduce=True`` runs
    ``lll_reduction`` first (test_cvp.cpp:43-58); the coefficients are then those in the reduced basis.
    ``ectx``: the context the enumerations run on (None: ``ctx``).  ``route``: "enum", "wave" or "auto", and
    ``max_nodes``, the node budget per target of the wave kernel (0: none; "auto": its built-in budget): see
    ``MatGSOBatch.closest_vector``.

    Returns ``(sol_coord, vectors)`` — int64 [T][d] and the lattice vectors sol_coord @ b as Python-int object arrays
    [T][n] — and with ``with_dist`` the enumeration's squared distances as a third item (to the
    target's projection on the span of ``b``: for d < n the part of the target orthogonal to the span is not in them).  A target whose numbers
    leave the int64 range raises ``HipError`` (the caller keeps the reference's multi-precision path)."""
    if route not in _lib.CVP_ROUTES:
        raise ValueError("closest_vectors: route is one of %s, got %r" % (", ".join(sorted(_lib.CVP_ROUTES)), route))
    if int(max_nodes) < 0:
        raise ValueError("closest_vectors: max_nodes is a node budget >= 0 (0: none), got %r" % (max_nodes,))
    b = np.ascontiguousarray(b, dtype=np.int64)
    if b.ndim != 2:
        raise ValueError("closest_vectors: b is [d][n]")
    t = np.ascontiguousarray(targets, dtype=np.int64)
    if t.ndim != 2 or t.shape[1] != b.shape[1]:
        raise ValueError("closest_vectors: targets are [T][%d], got shape %r" % (b.shape[1], t.shape))
    if reduce:
        b, _, status, _ = lll_reduction(ctx, b, with_u=False)
        if status != RED_SUCCESS:
            raise _lib.HipError("closest_vectors: lll_reduction ended with status %d" % status)
    g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1])
    try:
        g.set_basis(b)
        sol, dist, st = g.closest_vector(t, ectx=ectx, method=method, route=route, max_nodes=max_nodes)
    finally:
        g.close()
    bad = np.nonzero(st != RED_SUCCESS)[0]
    if len(bad):
        raise _lib.HipError("closest_vectors: target %d ended with status %d (-2: beyond the int64 range, -1: the "
                            "Babai loop found no fixed point, 2: the wave route's node budget ended the walk)" % (int(bad[0]), int(st[bad[0]])))
    vec = sol.astype(object).dot(b.astype(object))
    return (sol, vec, dist) if with_dist else (sol, vec)


def closest_vector(ctx, b, target, reduce=False, method=CVPM_FAST, ectx=None, with_dist=False, route="enum",
                   max_nodes=0):
    """One target: ``(sol_coord [d], vector [n])`` (and the squared distance with ``with_dist``); see
    ``closest_vectors``."""
    if route not in _lib.CVP_ROUTES:
        raise ValueError("closest_vector: route is one of %s, got %r" % (", ".join(sorted(_lib.CVP_ROUTES)), route))
    t = np.ascontiguousarray(target, dtype=np.int64)
    if t.ndim != 1:
        raise ValueError("closest_vector: target is one vector of n integers")
    out = closest_vectors(ctx, b, t[None], reduce=reduce, method=method, ectx=ectx, with_dist=with_dist, route=route,
                          max_nodes=max_nodes)
    return tuple(a[0] for a in out)
