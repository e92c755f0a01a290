"""python genie/novelty.py --indir out --refdir known_pdbs [--tm_threshold 0.5] [--norm query] ... (gapped TM alignment in HIP against
known structures, novelty)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genie2_amd.novelty import build_parser, check_args, main, reference_files, write_report  # noqa: E402,F401

if __name__ == '__main__':
    main(build_parser().parse_args())
