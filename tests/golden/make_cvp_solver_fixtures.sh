#!/bin/bash
# Regenerates tests/golden/cvpsolve_*.json with the REAL reference: lll_reduction + closest_vector (CVPM_FAST) recorded
# by tests/native/closest_vector_ref_driver.cpp — build line in its header, the binary goes to oracle/_ref/.  What the
# fixtures are for: tests/test_cvp_solver_cpu.py (their conditions) and tests/test_cvp_solver_gpu.py.
set -e
cd "$(dirname "$0")/../.."
D=oracle/_ref/closest_vector_ref_driver
G=tests/golden
#  d seed qbits targets...   (q-ary, q a prime of 11 bits: entries below 2^11)
# Every target must have ONE closest vector by a margin: a fixed-radius enumeration at 1.01 times the best squared
# distance holds exactly one candidate (tests/test_cvp_solver_cpu.py) — a seed that fails it is replaced, a tied
# instance has no single right answer.  far: entries around 2^40, the Babai loop runs more than once.
$D 24 1 11 rand rand near:6 lattice far:6  > $G/cvpsolve_q24.json
$D 36 2 11 near:8 near:10 lattice far:8    > $G/cvpsolve_q36.json
$D 40 3 11 near:8 near:10 lattice far:8    > $G/cvpsolve_q40.json
