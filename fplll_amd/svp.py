"""Shortest vectors, and lists of short and near lattice vectors: every vector within a radius, exactly.

What the reference does with a BEST_N evaluator that never fills (``FastEvaluator(999999)`` in its test_list_cvp; the
list behind ``shortest_vectors(..., max_sols)``): kissing numbers, theta series, list decoding.  Everything is computed
on the GPU behind ``fphip_list_vectors`` (include/fplll_hip.h): update_gso, a list enumeration that keeps every
candidate on the device (``fphip_enum_list``), the vector kernel (exact int64 vectors and norms) and the filter on the
exact integer norm; nothing here enumerates on the CPU.  Bases of at most 64 rows with int64 entries, one rank.

``shortest_vector`` / ``shortest_vector_batch`` are the reference's ``shortest_vector(b, sol_coord, SVPM_FAST)``
(``fplll -a svp``) behind ``fphip_shortest_vector``: a wave-per-lattice kernel for batches of bases of at most 64 rows,
the multi-wave enumerator for larger ones, the answer decided on exact integer norms on either route.

``shortest_vectors`` / ``shortest_vectors_batch`` are the reference's ``shortest_vectors(..., max_sols)`` as such: the
N <= 64 shortest vectors of every lattice of a batch under a radius that shrinks to the worst kept norm
(``fphip_shortest_vectors``), no radius to guess and no list to cut afterwards.
"""
import numpy as np

from . import _lib
from .gso import MatGSOBatch, lll_reduction

RED_SUCCESS = 1
DEFAULT_CAP = 1 << 18


def _basis(b, what):
    b = np.ascontiguousarray(b, dtype=np.int64)
    if b.ndim != 2 or b.shape[0] < 1 or b.shape[0] > b.shape[1]:
        raise ValueError("%s: b is [d][n] with 1 <= d <= n, got shape %r" % (what, b.shape))
    return b


def _list(ctx, b, target, bound_sq, reduce, cap, ectx, what):
    if int(bound_sq) != bound_sq or bound_sq < 0:
        raise ValueError("%s: bound_sq is a non-negative integer (the squared norms of an integer lattice are)" % what)
    if int(cap) < 0:
        raise ValueError("%s: cap cannot be negative" % what)
    u = None
    if reduce:
        b, u, status, _ = lll_reduction(ctx, b, with_u=True)
        if status != RED_SUCCESS:
            raise _lib.HipError("%s: lll_reduction ended with status %d" % (what, status))
    g = MatGSOBatch(ctx, 1, b.shape[0], b.shape[1])
    try:
        g.set_basis(b)
        count, coef, vec, norm = g.list_vectors(int(bound_sq), target=target, cap=int(cap), ectx=ectx)
    finally:
        g.close()
    if u is not None:  # v = coef (u b_in): the coefficients in the caller's basis, exact
        coef = coef.astype(object).dot(np.asarray(u).astype(object))
    return count, coef, vec, norm


def short_vectors(ctx, b, bound_sq, reduce=True, cap=DEFAULT_CAP, ectx=None):
    """Every non-zero vector v of the lattice spanned by the rows of ``b`` (int64 [d][n]) with |v|^2 <= bound_sq, one of
    each pair +-v.  ``reduce=True`` runs ``lll_reduction`` first (the enumeration expects a reduced basis) and expresses
    the coefficients in the caller's basis through u.  Returns ``(count, coef [m][d], vec [m][n], norm [m])`` with
    m = min(count, cap): ``count`` is exact whatever ``cap`` is; the rows come sorted by norm."""
    return _list(ctx, _basis(b, "short_vectors"), None, bound_sq, reduce, cap, ectx, "short_vectors")


def vectors_near(ctx, b, target, bound_sq, reduce=True, cap=DEFAULT_CAP, ectx=None):
    """Every lattice vector w with |w - target|^2 <= bound_sq (``target`` int64 [n]; a target in the lattice is found at
    norm 0).  Returns ``(count, coef, vec, norm)`` like ``short_vectors``; ``vec`` holds w - target, so the lattice
    vectors themselves are ``vec + target``."""
    b = _basis(b, "vectors_near")
    t = np.ascontiguousarray(target, dtype=np.int64)
    if t.shape != (b.shape[1],):
        raise ValueError("vectors_near: target is [%d], got shape %r" % (b.shape[1], t.shape))
    return _list(ctx, b, t, bound_sq, reduce, cap, ectx, "vectors_near")


def theta_series(ctx, b, bound_sq, reduce=True, ectx=None):
    """``{norm: number of lattice vectors of that squared norm}`` for the norms 0 < norm <= bound_sq, both signs
    counted (a kissing number is the entry of the minimum)."""
    count, _, _, norm = short_vectors(ctx, b, bound_sq, reduce=reduce, cap=DEFAULT_CAP, ectx=ectx)
    if count > len(norm):
        count, _, _, norm = short_vectors(ctx, b, bound_sq, reduce=reduce, cap=count, ectx=ectx)
    vals, cnts = np.unique(norm, return_counts=True)
    return {int(v): 2 * int(c) for v, c in zip(vals, cnts)}


def shortest_vector_batch(ctx, bs, reduce=True, pruning=None, route="auto", ectx=None):
    """A shortest non-zero vector of every lattice of ``bs`` (int64 [B][d][n], rows = basis vectors):
    shortest_vector(b, sol_coord, SVPM_FAST) of the reference, one call for the batch.  ``reduce=True`` runs the batched
    LLL first (the enumeration expects a reduced basis) and expresses ``sol_coord`` in the caller's basis through u, in
    exact Python integers.  ``pruning``: [d] level coefficients or None; ``route``: "auto", "wave" (one wavefront per
    lattice, d <= 64, deterministic) or "enum" (one enumerator call per lattice, on ``ectx``).  Returns ``(sol_coord
    [B][d], vec int64 [B][n], norm int64 [B])`` with vec = sol_coord b and norm = |vec|^2 exactly; ``sol_coord`` is
    int64 without ``reduce`` and an object array of Python integers with it.  Raises ``HipError`` naming the lattice
    where a status is not RED_SUCCESS."""
    b = np.ascontiguousarray(bs, dtype=np.int64)
    if b.ndim != 3 or b.shape[0] < 1 or b.shape[1] < 1 or b.shape[1] > b.shape[2]:
        raise ValueError("shortest_vector_batch: bs is [B][d][n] with B >= 1 and 1 <= d <= n, got shape %r" % (b.shape,))
    if route not in _lib.SVP_ROUTES:
        raise ValueError("shortest_vector_batch: route is one of %s, got %r" % (", ".join(sorted(_lib.SVP_ROUTES)), route))
    if pruning is not None and np.shape(pruning) != (b.shape[1],):
        raise ValueError("shortest_vector_batch: pruning is [%d], got shape %r" % (b.shape[1], np.shape(pruning)))
    g = MatGSOBatch(ctx, b.shape[0], b.shape[1], b.shape[2])
    try:
        g.set_basis(b)
        u = None
        if reduce:
            g.enable_transform()
            status, _ = g.lll()
            for k, s in enumerate(status):
                if s != RED_SUCCESS:
                    raise _lib.HipError("shortest_vector: lll of lattice %d ended with status %d" % (k, s))
            u = g.get_transform()
        sol, vec, norm, _, status = g.shortest_vector(pruning=pruning, route=route, ectx=ectx)
    finally:
        g.close()
    for k, s in enumerate(status):
        if s != RED_SUCCESS:
            raise _lib.HipError("shortest_vector: lattice %d ended with status %d (%s)" % (
                k, s, "an entry or a norm beyond 63 bits" if s == -2 else "update_gso failed"))
    if u is not None:  # v = sol (u b_in): the coefficients in the caller's basis, exact
        sol = np.stack([sol[k].astype(object).dot(u[k].astype(object)) for k in range(len(sol))])
    return sol, vec, norm


def shortest_vector(ctx, b, reduce=True, pruning=None, route="auto", ectx=None):
    """``shortest_vector_batch`` for one basis ``b`` (int64 [d][n]): ``(sol_coord [d], vec [n], norm)``."""
    b = _basis(b, "shortest_vector")
    sol, vec, norm = shortest_vector_batch(ctx, b[None], reduce=reduce, pruning=pruning, route=route, ectx=ectx)
    return sol[0], vec[0], int(norm[0])


def shortest_vectors_batch(ctx, bs, max_sols, bound_sq=None, reduce=True, pruning=None, route="auto", ectx=None):
    """The ``max_sols`` (1 .. 64) shortest non-zero vectors, one of each pair +-v, of every lattice of ``bs`` (int64
    [B][d][n]): the reference's shortest_vectors(max_sols), one call for the batch.  ``bound_sq``: None (per lattice the
    norm of its shortest row after the reduction: at least one vector is found), one non-negative integer, or [B] of
    them (0 = the default); only vectors with norm <= the bound are kept, so fewer than ``max_sols`` may come back.
    ``reduce=True`` runs the batched LLL first and expresses ``sol_coord`` in the caller's basis through u, in exact
    Python integers.  ``pruning`` and ``route`` as in ``shortest_vector_batch``; on the "wave" route the answer is the
    first max_sols vectors in (norm, depth-first discovery) order, on "enum" which of several vectors tied at the cut
    are kept is unspecified.  Returns ``(found int32 [B], sol_coord [B][max_sols][d], vec int64 [B][max_sols][n], norm
    int64 [B][max_sols])``, sorted by norm, entries beyond ``found`` zero.  With ``pruning`` a lattice may have found =
    0 (the reference's RED_ENUM_FAILURE); raises ``HipError`` naming the lattice where a status is not RED_SUCCESS."""
    b = np.ascontiguousarray(bs, dtype=np.int64)
    if b.ndim != 3 or b.shape[0] < 1 or b.shape[1] < 1 or b.shape[1] > b.shape[2]:
        raise ValueError("shortest_vectors_batch: bs is [B][d][n] with B >= 1 and 1 <= d <= n, got shape %r" % (b.shape,))
    if int(max_sols) != max_sols or not 1 <= max_sols <= 64:
        raise ValueError("shortest_vectors_batch: max_sols is an integer in 1 .. 64, got %r (longer lists: short_vectors)" % (max_sols,))
    if route not in _lib.SVP_ROUTES:
        raise ValueError("shortest_vectors_batch: route is one of %s, got %r" % (", ".join(sorted(_lib.SVP_ROUTES)), route))
    if pruning is not None and np.shape(pruning) != (b.shape[1],):
        raise ValueError("shortest_vectors_batch: pruning is [%d], got shape %r" % (b.shape[1], np.shape(pruning)))
    if bound_sq is not None:
        bq = np.asarray(bound_sq)
        if bq.shape not in ((), (b.shape[0],)) or any(int(v) != v or v < 0 for v in bq.reshape(-1).tolist()):
            raise ValueError("shortest_vectors_batch: bound_sq is None, a non-negative integer or [%d] of them, got %r" % (b.shape[0], bound_sq))
    g = MatGSOBatch(ctx, b.shape[0], b.shape[1], b.shape[2])
    try:
        g.set_basis(b)
        u = None
        if reduce:
            g.enable_transform()
            status, _ = g.lll()
            for k, s in enumerate(status):
                if s != RED_SUCCESS:
                    raise _lib.HipError("shortest_vectors: lll of lattice %d ended with status %d" % (k, s))
            u = g.get_transform()
        found, sol, vec, norm, _, status = g.shortest_vectors(int(max_sols), bound_sq=bound_sq, pruning=pruning, route=route, ectx=ectx)
    finally:
        g.close()
    for k, s in enumerate(status):
        if s != RED_SUCCESS:
            raise _lib.HipError("shortest_vectors: lattice %d ended with status %d (%s)" % (
                k, s, "an entry or a norm beyond 63 bits" if s == -2 else "update_gso failed"))
    if u is not None:  # v = sol (u b_in): the coefficients in the caller's basis, exact
        sol = np.stack([sol[k].astype(object).dot(u[k].astype(object)) for k in range(len(sol))])
    return found, sol, vec, norm


def shortest_vectors(ctx, b, max_sols, bound_sq=None, reduce=True, pruning=None, route="auto", ectx=None):
    """``shortest_vectors_batch`` for one basis ``b`` (int64 [d][n]) and one ``bound_sq`` (None or an integer):
    ``(found, sol_coord [max_sols][d], vec [max_sols][n], norm [max_sols])``."""
    b = _basis(b, "shortest_vectors")
    if bound_sq is not None and np.ndim(bound_sq) != 0:
        raise ValueError("shortest_vectors: bound_sq is None or one non-negative integer, got %r" % (bound_sq,))
    found, sol, vec, norm = shortest_vectors_batch(ctx, b[None], max_sols, bound_sq=bound_sq, reduce=reduce, pruning=pruning,
                                                   route=route, ectx=ectx)
    return int(found[0]), sol[0], vec[0], norm[0]
