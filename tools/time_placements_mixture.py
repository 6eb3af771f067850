#!/usr/bin/env python
"""
Query placements under a site-class mixture over K rate sets (state queries on every branch, sums
only): milliseconds per evaluation of the whole alignment, by

  mixture    place_queries_mixture(per_site=False) of one ordinary batch under the resident rate
             sets
  separate   K x (set_rates + step + place_queries(per_site=True)) of the same batch, one
             step_multi + fetch_multi_log_likelihoods, and the combination in numpy on the host
  single     one single-set place_queries(per_site=False) call

for the rows `small` (16 queries, 1 fraction, 1 pendant length) and `large` (64 queries, 3
fractions, 4 pendant lengths; the separate form holds K per-site arrays of nsites x 64 x nnodes x
12 doubles on the host), measured and reported as tools/time_spr_scores_mixture.py does (the same
program with the other call: see there for the options).

    python tools/time_placements_mixture.py [c2|c3|c6] [--K 4] [--rows small,large]
        [--baseline-only] [--out profiles/placements_mixture_c3.json] [--once ROW]
        [--once-single ROW]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_spr_scores_mixture import main               # noqa: E402

if __name__ == '__main__':
    main('place')
