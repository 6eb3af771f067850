#!/usr/bin/env python
"""
Query placements with each site under its own rate set (site i in set i % K, sums only): 16 state
queries on every edge at the one fraction 0.5 and one pendant length: microseconds per evaluation
of the whole alignment under K fresh parameter vectors, by set_rate_sets +
place_queries_partitioned of ONE partitioned batch and by K x (set_rates + place_queries) over K
ordinary sub-batches (each with its set's slice of the queries) with the sums added on the host --
the program of time_branch_profiles_partitioned.py, whose options it takes.

    python tools/time_placements_partitioned.py --workload c3 --K 4,64
        [--baseline-only] [--single] [--out profiles/placements_partitioned_c3.json] [--once K]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_branch_profiles_partitioned import main          # noqa: E402

if __name__ == '__main__':
    main('place', (('16 state queries', None),))
