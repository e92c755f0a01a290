"""python genie/sample_unconditional_shape.py --name ... --rog_max ... (the unconditional flags plus the shape and secondary-structure terms)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genie2_amd.sample_unconditional_shape import (ShapeRunner, add_secstruct_arguments, build_parser, main,  # noqa: E402,F401
                                                   secstruct_constants, secstruct_potential)

if __name__ == '__main__':
    main(build_parser().parse_args())
