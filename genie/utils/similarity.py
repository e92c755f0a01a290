from genie2_amd.similarity import (PairwiseTM, cluster_leader, cluster_single, diversity_summary, load_designs,  # noqa: F401
                                   seed_windows, tm_d0)
