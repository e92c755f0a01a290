from genie2_amd.similarity import (PairwiseTM, TMAlign, align_sets, cluster_leader, cluster_single, diversity_summary,  # noqa: F401
                                   length_chunks, load_designs, plan_calls, seed_windows, tm_d0)
