#!/bin/bash
# Regenerates tests/golden/cvpw_*.json.gz with the REAL reference: closest-vector enumerations of blocks ABOVE 64 rows
# (Enumeration::enumerate with a target) recorded by tests/native/cvp_ref_driver.cpp — build line in its header, the
# binary goes to oracle/_ref/.  Each fixture meets the conditions tests/test_enum_cvp_wide_cpu.py asserts: 10^4 ..
# 3 10^6 nodes in all, a level >= 64 with at least 3 nodes, no more level-64 nodes than the top task buffer holds, a
# candidate, and the shortest candidate passes every pruned bound under its own distance.
set -e
cd "$(dirname "$0")/../.."
D=oracle/_ref/cvp_ref_driver
G=tests/golden
#    d  seed slope radius     pruning   target
# a real target under the Gaussian-heuristic radius (a flat profile: the tree of a steep one at 72 rows is out of
# reach), pruned; the rounding descent leaves the radius at level 20
$D  72 1 0.005 gh:1       stair:0.5 real          | gzip -9n > $G/cvpw_d72_real.json.gz
# the target IS the lattice point 3 b_71: distance exactly 0
$D  72 1 0.03  gh:0.2     stair:0.5 lattice       | gzip -9n > $G/cvpw_d72_lattice.json.gz
# a target near a lattice point, moved by 0.6 along row 80 / 100: the rounding descent takes the wrong neighbour
# there and leaves the radius (a twentieth / a hundredth of its own distance) ABOVE level 64 — k0 = 65 and 93: the
# counting compensation stops above level 64; d = 136: four registers per lane, the column stack in global memory
$D  96 1 0.02  babai:0.05 none      bump:80:0.6   | gzip -9n > $G/cvpw_d96_k0.json.gz
$D 136 1 0.02  babai:0.01 none      bump:100:0.6  | gzip -9n > $G/cvpw_d136_k0.json.gz
