"""python genie/sample_unconditional_shape.py --name ... --rog_max ... (the unconditional flags plus the shape, secondary-structure,
sheet, symmetry, binder, fold, diversity, burial and envelope terms)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genie2_amd.sample_unconditional_shape import (ShapeRunner, add_binder_arguments, add_burial_arguments, add_diversity_arguments, add_envelope_arguments,  # noqa: E402,F401
                                                   add_fold_arguments, add_secstruct_arguments, add_sheet_arguments, add_symmetry_arguments,
                                                   binder_constants, binder_potential, build_parser, burial_constants, burial_potential, diversity_constants, envelope_constants, envelope_potential,
                                                   diversity_potential, fold_constants, fold_potential, main, secstruct_constants,
                                                   secstruct_potential, sheet_constants, sheet_potential, symmetry_constants,
                                                   symmetry_potential)

if __name__ == '__main__':
    main(build_parser().parse_args())
