#!/usr/bin/env python
"""
NNI scores under a site-class mixture over K rate sets (all moves, the plain swap and 8 factors of
the edge above v, sums only): milliseconds per evaluation of the whole alignment, by

  mixture    nni_scores_mixture(per_site=False) of one ordinary batch under the resident rate sets
  separate   K x (set_rates + step + nni_scores(per_site=True)) of the same batch, one step_multi +
             fetch_multi_log_likelihoods, and the combination in numpy on the host

measured and reported as tools/time_branch_profiles_mixture.py does (the same program with the
other call: see there for the options).

    python tools/time_nni_scores_mixture.py [c2|c3|c6] [--K 4] [--baseline-only]
        [--out profiles/nni_scores_mixture_c3.json] [--once] [--once-single]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_branch_profiles_mixture import main          # noqa: E402

if __name__ == '__main__':
    main('nni')
