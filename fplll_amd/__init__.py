"""fplll_amd — MI355X-native (gfx950, HIP) implementation of fplll's GSO / SVP-enumeration hot path.

Only what the path needs lives here: ``csrc/`` (HIP kernels + the C ABI of include/fplll_hip.h +
the host C++ adapter for fplll's external-enumerator hook) and a thin Python mirror of the
reference interface used by tests and bench.  See DESIGN.md / INTEGRATION.md.
"""
from ._lib import Context, HipError, load, LIB_PATH  # noqa: F401
from .enumeration import (  # noqa: F401
    EVALSTRATEGY_BEST_N_SOLUTIONS, EVALSTRATEGY_FIRST_N_SOLUTIONS,
    EVALSTRATEGY_OPPORTUNISTIC_N_SOLUTIONS, FastEvaluator, Unsupported, enumerate_block)
from .cvp import closest_vector, closest_vectors  # noqa: F401
from .svp import (short_vectors, shortest_vector, shortest_vector_batch, shortest_vectors,  # noqa: F401
                  shortest_vectors_batch, theta_series, vectors_near)
from .gram import (MatGSOGramBatch, lll_reduction_gram, shortest_vector_gram, shortest_vectors_gram,  # noqa: F401
                   sqnorm_coordinates)
