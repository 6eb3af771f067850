#!/usr/bin/env python
"""
SPR scores with each site under its own rate set (site i in set i % K, sums only), every move
within radius 1 and within radius 3 at the one fraction 0.5: microseconds per evaluation of the
whole alignment under K fresh parameter vectors, by set_rate_sets + spr_scores_partitioned of ONE
partitioned batch and by K x (set_rates + spr_scores) over K ordinary sub-batches with the sums
added on the host -- the program of time_branch_profiles_partitioned.py, whose options it takes.

    python tools/time_spr_scores_partitioned.py --workload c3 --K 4,64
        [--baseline-only] [--single] [--out profiles/spr_scores_partitioned_c3.json] [--once K]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_branch_profiles_partitioned import main          # noqa: E402

if __name__ == '__main__':
    main('spr', (('radius 1', 1), ('radius 3', 3)))
