#!/bin/bash
# Regenerates tests/golden/cvp_*.json with the REAL reference: closest-vector enumerations
# (Enumeration::enumerate with a target) recorded by tests/native/cvp_ref_driver.cpp — build line in its header,
# the binary goes to oracle/_ref/.  What each fixture is for: tests/test_enum_cvp_gpu.py.
set -e
cd "$(dirname "$0")/../.."
D=oracle/_ref/cvp_ref_driver
G=tests/golden
#    d seed slope radius     pruning    target
# general position, real targets.  d20: the rounding descent stays within the radius (k0 = 0); d32: the radius is 0.72
# of that descent's distance (k0 > 0); d40_stair: the descent fails the pruned bound of a level ABOVE the one where it
# leaves the radius — the reference still takes a node off that level.  The seeds of the pruned ones are chosen so
# that the shortest candidate passes every pruned bound under its OWN distance as the radius: a BEST_N(1) run then ends
# on it whatever the order of the walk (tests/test_enum_cvp_gpu.py asserts that precondition)
$D 20 1 0.045 gh:1.5     none       real          > $G/cvp_d20_real.json
$D 32 2 0.045 babai:0.72 none       real          > $G/cvp_d32_real_k0.json
$D 40 3 0.045 gh:1.1     none       real          > $G/cvp_d40_real.json
$D 32 12 0.045 gh:1.4    stair:0.25 real          > $G/cvp_d32_stair.json
$D 40 21 0.045 gh:1.15   stair:0.5  real          > $G/cvp_d40_stair.json
# the target IS the lattice point 3 b_31 (distance exactly 0), and a target within 1e-3 of it
$D 32 6 0.045 gh:1.05    none       lattice       > $G/cvp_d32_lattice.json
$D 32 7 0.045 gh:1.05    none       near:1e-4     > $G/cvp_d32_near.json
# the rounding descent stays within the radius but fails the pruned bound of level 20 (the unchecked decrement)
$D 40 9 0.045 babai:1.5  stair:0.25 bump:20:0.49  > $G/cvp_d40_stair_bump.json
