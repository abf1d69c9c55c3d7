// enum_walk4.hip — the fourth generation of the walk launches: enum_walk4_kernel<MU_LDS, DUAL>.  The text of
// enum_walk.hip compiled with FPHIP_WALK4 = 1 (see the header there, and DESIGN.md section 3).  The kernel of the final
// walk launches of shortest-vector calls; FPHIP_WALK4=0 launches the third generation, its A/B partner.  Closest-vector
// and sub-solution calls keep their kernels.
//
// The fourth generation is the third — the masks P and B, chain descents that store nothing, the row broadcast, the
// tie test on the descent with siblings: same visit set, arithmetic, counting rule and candidates — with one change.
//
//     Ready pair siblings (FPHIP_W4_PAIR).  16 % of the visited nodes of the flagship tree have exactly two children.
//     For the second one the third generation stores (c, x_0, pd, st) and the parent's column at the descent, and at the
//     STEP fetches them back (a readlane, six bpermutes, the (r, pruning) pair, the mu row, the stack slot) to run a
//     dependent chain of seven double-precision operations.  Every operand of that chain is in registers at the
//     descent.  So a descent whose ballot counts two children (popcount 5) forms the sibling there:
//         s = (c >= x_0) ? +1 : -1  (x_0 after the tie correction: the test STEP makes)
//         x_2 = x_0 + s;  a_2 = x_2 - c;  nd_2 = nd + a_2 a_2 r;  S_2 = S - (DUAL ? a_2 : x_2) mu_k
//     STEP forms x = fma(z, sgd, x_0) with z = 1, sgd = +-1: the one rounding of x_0 + s, which x_0 + s is as well;
//     then a = x - c, nd = pd + a a r (pd = the parent's nd, r the scalar load of the same table entry — the
//     expansion's (r, pruning) pair holds the same double), S = par - (DUAL ? a : x) mk with par = the pushed S and
//     mk = the same row of mu, fetched with the same clamp.  Separate multiplies and adds in the same order on the
//     same operands: every double of the sibling is bit for bit the one STEP forms (tests/test_walk_pair_model.py).
//     Stored: S_2 in the slot of the push (LDS or, above the split, global), nd_2 in lane k of pds, x_2 in lane k of
//     x0s; P and the pair mask Q are set, B is cleared — below the first child the level is a level outside B, its
//     coefficient roundto(centre) for the path replay.  The pair STEP pops S, broadcasts nd (one bpermute pair),
//     clears P and sets B; B with Q says "the coefficient is lane k of x0s" (the lane's c and st are stale and not
//     read).  Reprune tests lane k of pds against the new bound and clears P and Q where it fails; a pending pair
//     sibling at an emission level is stepped to like any other and donated with (popped column, x_2, nd_2).  Nodes
//     with three or more children, slow levels, the zero chain and the special levels keep the third generation's path.
//
// Measured and not kept: node counts per run of EXPAND — one v_addc of a bit range where a run
// ends instead of one per link and step.  Alone it bought nothing (-0.3 %), beside the pairs it cost 0.4 %.
//
// Build: the flags of enum_walk.hip.
#define FPHIP_WALK4 1
#include "enum_walk.hip"
