#!/bin/sh
# The cost of weights and of the covariance kernel on the batched path, both precisions: one process per precision, each under
# its own time limit, chained so that nothing starts after a failure. Run from the repository root on the GPU box; the lines go
# to standard output (profiles/r08/batched_weighted.txt holds a run).
set -e
timeout -k 10 240 python scripts/batched_weighted_cost.py f32 &&
timeout -k 10 240 python scripts/batched_weighted_cost.py f64
