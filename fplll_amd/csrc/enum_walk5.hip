// enum_walk5.hip — the fifth generation of the walk launches: enum_walk5_kernel<MU_LDS, DUAL>.  The text of
// enum_walk.hip compiled with FPHIP_WALK5 = 1 (see the header there, and DESIGN.md section 3).  The kernel of the final
// walk launches of shortest-vector calls; FPHIP_WALK5=0 launches the fourth generation, its A/B partner.
//
// The fifth generation is the fourth — masks P, B and Q, chain descents that store nothing, ready pair siblings: same
// visit set, arithmetic, counting rule, candidates and stored state — with two changes.  A wave's time per node is the
// length of its own instruction sequence with the waits in it, not the vector port: both changes
// shorten that sequence.
//
//  1. The pair descent reads its sibling off the test (FPHIP_W5_PAIR).  The fourth generation formed the second child of
//     a two-child node by STEP's sequence: a compare and a select for the direction, x_2 = x_0 +- 1, a_2 = x_2 - c,
//     nd_2 = nd + a_2 a_2 r.  Without a tie that child IS the test's candidate z = +1 or z = -1 — the nearer neighbour
//     of x_0, z = +1 iff c > x_0, which is the direction STEP takes — and its distance is ndj of that lane: a1 + z and
//     (x_0 + z) - c are the same double (tests/test_walk_bcast_model.py), everything after that is STEP's sequence
//     (tests/test_walk5_model_cpu.py).  For that distance to reach the level's lane by a row broadcast, as the first
//     child's does, EVERY row must hold the two neighbours (row_newbcast reads within a 16-lane row, and the level's
//     lane may be in any): the candidate layout of this generation is z = 0, +1, -1 in lanes 0, 1, 2 of every row and
//     +-2 ... +-27 over the other 52 lanes — 55 distinct candidates, not 61.  A two-child node has popcount 8; the
//     number of children of a wider node is the popcount of the ballot without the copies (FPHIP_ZONCE); a node whose
//     55 candidates all survive takes the general path, as one with 61 did.  The direction is bit 1 of the ballot (a
//     uniform branch), x_2 = x_0 +- 1.0 an inline constant, nd_2 one DPP move (row_bcast_f64<1 / 2>, enum_wave.h): one
//     vector instruction where there were six.  A tie (|a1| = 0.5: both neighbours share a distance, the direction
//     comes from roundto's correction) keeps the fourth generation's computation in a block of its own.
//
//  2. The EXPAND loop rotated (FPHIP_W5_AHEAD).  What a level's test waits for — the centre's broadcast through the LDS
//     crossbar, the (r, pruning) pair through the scalar cache, the mu row — was asked for at the top of the level's
//     iteration, behind the bookkeeping of the descent that led there.  Now every descent forms the child's column
//     first and asks at once (FPHIP_NEXT_LEVEL); the count, the DPP move of the child's distance, the masks and the
//     selects of the descent run while the answers travel.  Same instructions on the same operands in another order;
//     what a descent asked for in vain (the test fails, a special level) is dropped, as the top of the loop's was.
//
// Measured and not kept: the first child's distance added by v_fmac_f64 with row_newbcast:0 on its
// factor, in place of the DPP move and the add — the result lands in the addend's register while the loop carries the
// distance in another, so the compiler puts a v_mov_b64 where the DPP move was: no instruction less, two s_nop more,
// 2 % slower.  The DPP moves without their s_nop (the hazard cannot arise behind the compare and the scalar tests):
// nothing.
//
// Build: the flags of enum_walk.hip.
#define FPHIP_WALK5 1
#include "enum_walk.hip"
