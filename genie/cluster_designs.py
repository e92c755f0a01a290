"""python genie/cluster_designs.py --indir out [--tm_threshold 0.6] [--linkage single|leader] ... (pairwise TM-score in HIP, clusters,
diversity)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genie2_amd.cluster_designs import build_parser, check_args, design_files, main, score  # noqa: E402,F401

if __name__ == '__main__':
    main(build_parser().parse_args())
