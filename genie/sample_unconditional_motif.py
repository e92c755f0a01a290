"""python genie/sample_unconditional_motif.py --name ... --motif_file ... (the reference's flags plus the motif input)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genie2_amd.sample_unconditional_motif import MotifRunner, build_parser, main  # noqa: E402,F401

if __name__ == '__main__':
    main(build_parser().parse_args())
