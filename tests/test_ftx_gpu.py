"""fplll_amd/csrc/ftx.h ON THE DEVICE, in both extended types (double-double and quad-double, the stand-ins for
FP_NR<dd_real> / FP_NR<qd_real>), through fphip_debug_ftx_op (ftx_op_kernel, hlll_x.hip):

  1. every element-wise operation on the operands of tests/ftx_cases.py — the list tests/test_ftx_cpu.py runs on the
     host build — against mpmath with the same gates, and BIT FOR BIT equal to the host build of the same header:
     the library is compiled without contraction and without fast-math, and double + - * / fma sqrt floor ldexp are
     correctly rounded on both sides, so there is no tolerance;
  2. the wave-level helpers, which the host build cannot run (it stubs the shuffles): f_bcast / f_shfl_up / f_shfl_xor
     move every component of every lane unchanged, f_wave_sum leaves the same bits in all 64 lanes and is within
     6 units (six butterfly levels of one "sloppy" addition each) of the exact sum, relative to sum |a_i|.
"""
import ctypes

import numpy as np
import pytest

import conftest as C
import ftx_cases as F

pytestmark = pytest.mark.gpu
mp = pytest.importorskip("mpmath")

TYPES = pytest.mark.parametrize("comps", [4, 2], ids=["quad-double", "double-double"])


def _ftx_op(ctx, comps, op, a, b, expect=0):
    """a, b: [n][4] operands -> [n][4] results (components beyond `comps` zero)"""
    import fplll_amd
    lib = fplll_amd.load()
    vp = ctypes.c_void_p
    lib.fphip_debug_ftx_op.restype = ctypes.c_int
    lib.fphip_debug_ftx_op.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    n = a.shape[0]
    pa = np.ascontiguousarray(np.asarray(a, dtype=np.float64)[:, :comps].T)   # planes [comps][n]
    pb = np.ascontiguousarray(np.asarray(b, dtype=np.float64)[:, :comps].T)
    po = np.full((comps, n), np.nan)
    rc = lib.fphip_debug_ftx_op(ctx.handle, comps, op, n, pa.ctypes.data, pb.ctypes.data, po.ctypes.data)
    assert rc == expect, (rc, ctx.last_error())
    out = np.zeros((n, 4))
    out[:, :comps] = po.T
    return out


def _same_bits(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return F.host_harness(tmp_path_factory.mktemp("ftx"))


@TYPES
def test_device_arithmetic_against_mpmath_and_the_host_build(ctx, host, comps):
    """2048 operands per operation over all operand classes: the mpmath gates of the host test (1 / 1 / 4 / 8 / 4 / 4
    units of 2^-205 or 2^-104, nint / le / gt / rnd_we exact, results normalised), and every result plane identical
    to the host build's, bit for bit."""
    for label, op, a, b, verify in F.checks(comps):
        out = _ftx_op(ctx, comps, op, a, b)
        line = verify(out)
        C.note(lambda: ("device %s %s" % ("qd" if comps == 4 else "dd", line),))
        ref = host(comps, op, a, b)
        diff = np.nonzero(np.any(out.view(np.uint64) != ref.view(np.uint64), axis=1))[0]
        assert diff.size == 0, (comps, label, "%d results differ from the host build" % diff.size,
                                [float(t).hex() for t in a[diff[0]]], [float(t).hex() for t in b[diff[0]]],
                                [float(t).hex() for t in out[diff[0]]], [float(t).hex() for t in ref[diff[0]]])


@TYPES
def test_wave_shuffles_move_every_component(ctx, comps):
    """f_bcast, f_shfl_up and f_shfl_xor on 32 wavefronts of distinct four- (two-) component values: every component
    of the source lane arrives unchanged; lane 0 of f_shfl_up keeps its own value; a count that is no multiple of 64
    is refused."""
    n = 2048
    a, _, _ = F.arith_cases(7, comps, n)
    a = a.copy()
    lane, wave = np.arange(n) % 64, np.arange(n) // 64
    rng = np.random.default_rng(17)
    b = np.zeros((n, 4))
    # f_bcast: a source lane per LANE (a gather); beyond 63 to see the `& 63`
    b[:, 0] = rng.integers(0, 256, n)
    out = _ftx_op(ctx, comps, 11, a, b)
    assert _same_bits(out, a[wave * 64 + (b[:, 0].astype(np.int64) & 63)])
    # ... and the kernels' use of it: one source lane for the whole wavefront
    b[:, 0] = (wave * 5 + 3) % 64
    out = _ftx_op(ctx, comps, 11, a, b)
    assert _same_bits(out, a[wave * 64 + b[:, 0].astype(np.int64)])
    # f_shfl_up by one lane
    out = _ftx_op(ctx, comps, 12, a, b)
    assert _same_bits(out, a[np.where(lane == 0, np.arange(n), np.arange(n) - 1)])
    # f_shfl_xor: every mask the butterflies use and the others, one per wavefront
    b[:, 0] = np.array([1, 2, 4, 8, 16, 32] + list(range(0, 256, 10)))[wave]
    out = _ftx_op(ctx, comps, 13, a, b)
    assert _same_bits(out, a[wave * 64 + (lane ^ (b[:, 0].astype(np.int64) & 63))])
    for op in (10, 11, 12, 13):
        _ftx_op(ctx, comps, op, a[:100], b[:100], expect=-1)


@TYPES
def test_wave_sum(ctx, comps):
    """f_wave_sum (the tree sum behind every dot product and norm of hlll_x.hip / lll_x.hip) on 32 wavefronts: mixed
    signs and magnitudes, one wavefront of 63 zeros and one value, one of exact cancellation.  All 64 lanes end with
    the same bits, and |got - sum a_i| <= 6 u sum |a_i| with u = 2^-205 (2^-104): six levels, each addition within one
    unit of its larger operand, which sum |a_i| bounds."""
    mp.mp.prec = F.PREC
    a = F.wave_cases(5, comps, 32)
    out = _ftx_op(ctx, comps, 10, a, a)
    u = mp.mpf(2) ** -F.EPS_BITS[comps]
    worst = mp.mpf(0)
    for w in range(32):
        lanes = out[64 * w:64 * w + 64]
        assert all(_same_bits(lanes[0], lanes[k]) for k in range(64)), w
        vals = [F.val(x) for x in a[64 * w:64 * w + 64]]
        want, mag = mp.fsum(vals), mp.fsum(abs(v) for v in vals)
        err = abs(F.val(lanes[0]) - want)
        assert err <= 6 * u * mag, (comps, w, mp.nstr(err / (u * mag), 5))
        worst = max(worst, err / (u * mag))
    assert _same_bits(out[64], a[64 + 37])           # 63 zeros and one value: that value, untouched
    assert not out[128:192].any()                    # exact cancellation: exactly zero
    bad, _ = F.normalisation(out, comps)
    assert not bad, bad[:4]
    C.note(lambda: ("device %s wave sum: worst error %s of 6 units of 2^-%d of sum |a_i|"
                    % ("qd" if comps == 4 else "dd", mp.nstr(worst, 3), F.EPS_BITS[comps]),))
