"""ctypes binding of libgenie_hip.so (include/genie_hip.h).

The library is the product path: importing this module builds nothing and
falls back to nothing -- if the shared object is missing or a symbol is absent
it raises, loudly.
"""
import ctypes as C
import os

# PyTorch-ROCm bundles its own libamdhip64; it must be the HIP runtime of the
# process (streams and device pointers are shared with torch), so it has to be
# loaded before libgenie_hip.so resolves the same SONAME.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('GENIE_HIP_LIB', os.path.join(_HERE, 'lib', 'libgenie_hip.so'))


class GenieDims(C.Structure):
    """genie_dims_t -- field order is the ABI."""
    _fields_ = [
        ('c_s', C.c_int32), ('c_p', C.c_int32),
        ('c_pos_emb', C.c_int32), ('c_chain_emb', C.c_int32), ('c_timestep_emb', C.c_int32),
        ('relpos_k', C.c_int32),
        ('template_dist_n_bin', C.c_int32),
        ('template_dist_min', C.c_float), ('template_dist_step', C.c_float),
        ('n_pair_transform_layer', C.c_int32), ('c_hidden_mul', C.c_int32), ('pair_transition_n', C.c_int32),
        ('n_structure_layer', C.c_int32), ('n_structure_block', C.c_int32),
        ('c_hidden_ipa', C.c_int32), ('n_head_ipa', C.c_int32), ('n_qk_point', C.c_int32), ('n_v_point', C.c_int32),
        ('rescale', C.c_float),
        ('n_timestep', C.c_int32), ('max_n_res', C.c_int32), ('max_n_chain', C.c_int32),
        ('c_hidden_tri_att', C.c_int32), ('n_head_tri', C.c_int32),      # zero tail = no triangular attention
    ]


class GenieFeatures(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in (
        'aatype', 'atom_positions', 'residue_mask', 'residue_index', 'chain_index',
        'fixed_sequence_mask', 'fixed_structure_mask', 'interface_mask')]


class GenieTaps(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ('s', 'p', 's_final', 'rots_out', 'trans_out', 'p_init', 'p_layer0', 'states', 'p_trimul_out0',
                                              'ipa_cat0', 'p_tri_att0')]


class GenieGemmDesc(C.Structure):
    """genie_gemm_desc_t (include/genie_hip.h): one strided, batched GEMM of the training path."""
    _fields_ = [(n, C.c_int32) for n in ('M', 'N', 'K', 'batch', 'nb2', 'nsplit', 'mode', 'terms', 'relu')] + \
               [(n, C.c_int64) for n in ('am', 'ak', 'bk', 'bn', 'cm', 'cn', 'a1', 'a2', 'b1', 'b2', 'c1', 'c2')] + [('alpha', C.c_float)] + \
               [('cblk', C.c_int32), ('cblk_m', C.c_int32), ('ctab', C.c_int64 * 8), ('atab', C.c_int64 * 8)]


class GenieTrainOpts(C.Structure):
    _fields_ = [('tri_dropout', C.c_float), ('ipa_dropout', C.c_float), ('transition_dropout', C.c_float), ('seed', C.c_uint32),
                ('train_mode', C.c_int32), ('fast_math', C.c_int32), ('struct_done_event', C.c_void_p)]


# name -> (restype, argtypes); every symbol include/genie_hip.h declares
SYMBOLS = {
    'genie_create': (C.c_int, [C.POINTER(GenieDims), C.c_int, C.POINTER(C.c_void_p)]),
    'genie_destroy': (None, [C.c_void_p]),
    'genie_last_error': (C.c_char_p, [C.c_void_p]),
    'genie_weight_count': (C.c_size_t, [C.POINTER(GenieDims)]),
    'genie_load_weights': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    'genie_set_tables': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'genie_prepare_features': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(GenieFeatures)]),
    'genie_frenet': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'genie_frenet_frames': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'genie_denoise': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.POINTER(GenieTaps)]),
    'genie_q_sample': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'genie_training_loss': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    'genie_adam_step': (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                  C.c_double, C.c_int]),
    'genie_train_forward_backward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_float, C.POINTER(GenieTrainOpts), C.c_void_p, C.c_void_p]),
    'genie_denoise_vjp': (C.c_int, [C.c_void_p] * 10),
    'genie_train_workspace_bytes': (C.c_size_t, [C.c_void_p]),
    'genie_train_kept_bytes': (C.c_size_t, [C.c_void_p]),
    'genie_train_gemm_flop': (C.c_double, [C.c_void_p]),
    'genie_train_gemm': (C.c_int, [C.c_void_p, C.POINTER(GenieGemmDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'genie_p_sample': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    'genie_sample_loop': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    'genie_reverse_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    'genie_sample_loop_steps': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'genie_set_math': (C.c_int, [C.c_void_p, C.c_int]),
    'genie_get_math': (C.c_int, [C.c_void_p]),
    'genie_profile_enable': (C.c_int, [C.c_void_p, C.c_int]),
    'genie_profile_read': (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                     C.POINTER(C.c_int64), C.c_int]),
    'genie_probe_mfma': (C.c_int, [C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    'genie_workspace_bytes': (C.c_size_t, [C.c_void_p]),
    'genie_motif_potential': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    'genie_motif_potential_work_bytes': (C.c_size_t, [C.c_int, C.c_int]),
    'genie_motif_potential_rigid': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_size_t]),
    'genie_motif_potential_rigid_work_bytes': (C.c_size_t, [C.c_int, C.c_int]),
    'genie_motif_potential_grouped': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    'genie_motif_potential_grouped_work_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'genie_smc_reweight': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_double] + [C.c_void_p] * 7 +
                           [C.c_size_t]),
    'genie_smc_reweight_work_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'genie_shape_potential': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float,
                                         C.c_int] + [C.c_void_p] * 10 + [C.c_size_t]),
    'genie_shape_potential_work_bytes': (C.c_size_t, [C.c_int, C.c_int]),
    'genie_secstruct_potential': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)] + [C.c_float] * 6 +
                                  [C.c_void_p, C.c_float] + [C.c_void_p] * 5),
    'genie_sheet_potential': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_float] * 4 + [C.c_int] * 2 + [C.c_float] * 6 +
                              [C.c_int] + [C.c_void_p] * 4 + [C.c_float] + [C.c_void_p] * 6 + [C.c_size_t]),
    'genie_sheet_potential_work_bytes': (C.c_size_t, [C.c_int, C.c_int]),
    'genie_symmetry_potential': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float] +
                                 [C.c_void_p] * 5 + [C.c_size_t]),
    'genie_symmetry_potential_work_bytes': (C.c_size_t, [C.c_int, C.c_int]),
    'genie_binder_potential': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p] + [C.c_float] * 8 +
                               [C.c_void_p] * 6 + [C.c_size_t]),
    'genie_binder_potential_work_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'genie_pairwise_tm': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'genie_fold_potential': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 +
                             [C.c_size_t]),
    'genie_fold_potential_work_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'genie_tm_align': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                 C.c_int, C.c_float] + [C.c_void_p] * 7),
    'genie_fold_align_potential': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_int, C.c_int, C.c_int, C.c_float, C.c_int] + [C.c_void_p] * 12 + [C.c_size_t]),
    'genie_fold_align_potential_work_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'genie_diversity_potential': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 6 +
                                  [C.c_size_t]),
    'genie_diversity_potential_work_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'genie_burial_potential': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 3 +
                               [C.c_float] * 3 + [C.c_void_p] * 6 + [C.c_size_t]),
    'genie_burial_potential_work_bytes': (C.c_size_t, [C.c_int, C.c_int]),
    'genie_envelope_potential': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_float] * 5 +
                                 [C.c_void_p] * 7 + [C.c_size_t]),
    'genie_envelope_potential_work_bytes': (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    'genie_context_potential': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] +
                                [C.c_float] * 6 + [C.c_void_p] * 6 + [C.c_size_t]),
    'genie_context_potential_work_bytes': (C.c_size_t, [C.c_int, C.c_int]),
}

MOTIF_MAX_GROUPS = 8       # GENIE_MOTIF_MAX_GROUPS of include/genie_hip.h
SHAPE_REPORT = ('rog', 'min_distance', 'n_clash', 'e_rog', 'e_clash', 'e_restraint', 'n_violated', 'max_violation')      # GENIE_SHAPE_REPORT slots

SECSTRUCT_REPORT = ('helix_content', 'extended_content', 'n_helix', 'n_extended', 'e_helix', 'e_extended', 'e_target',
                    'n_target_missed')      # GENIE_SECSTRUCT_REPORT slots
# P-SEA's C-alpha criteria (Labesse et al. 1997) for d2, d3, d4 and chi from ideal coordinates: H mu, H sigma, E mu, E sigma
SECSTRUCT_TABLE = (5.5, 5.3, 6.4, 0.77, 0.5, 0.5, 0.6, 0.25, 6.7, 9.9, 12.4, -0.12, 0.6, 0.9, 1.1, 0.45)

SHEET_REPORT = ('antiparallel_content', 'parallel_content', 'n_antiparallel', 'n_parallel', 'n_paired', 'e_antiparallel', 'e_parallel',
                'e_ladder', 'n_ladder_missed')      # GENIE_SHEET_REPORT slots
SHEET_COUNTS = ('n_antiparallel', 'n_parallel', 'n_paired', 'n_ladder_missed')
# ideal pleated-sheet geometry: mu_A, sigma_A, mu_P, sigma_P in Angstrom (neighbouring strands 4.8 A apart; antiparallel C-alpha pairs
# alternate around 4.5 / 5.5 A)
SHEET_TABLE = (5.0, 0.6, 4.8, 0.5)
SHEET_PARALLEL, SHEET_RUNG = 1 << 29, 1 << 30       # GENIE_SHEET_PARALLEL, GENIE_SHEET_RUNG: flags of a ladder table's partner words

SYMMETRY_REPORT = ('e_symmetry', 'symmetry_rmsd', 'rmsd_0', 'angle_0', 'rise_0', 'rmsd_1', 'angle_1', 'rise_1')      # GENIE_SYMMETRY_REPORT slots
SYMMETRY_MAX_GENERATORS = 2     # GENIE_SYMMETRY_MAX_GENERATORS

BINDER_REPORT = ('contacts', 'n_contacts', 'n_interface', 'target_min_distance', 'n_target_clash', 'n_hotspots_contacted', 'e_target_clash',
                 'e_contact', 'e_hotspot')      # GENIE_BINDER_REPORT slots
BINDER_COUNTS = ('n_contacts', 'n_interface', 'n_target_clash', 'n_hotspots_contacted')
BINDER_MAX_HOTSPOTS = 64        # GENIE_BINDER_MAX_HOTSPOTS

TM_SEEDS, TM_MIN_LENGTH, TM_MAX_LENGTH, TM_MAX_ITER = 11, 4, 1706, 32      # GENIE_TM_SEEDS, _MIN_LENGTH, _MAX_LENGTH, _MAX_ITER
TMALIGN_MAX_LENGTH, TMALIGN_MAX_CELLS, TMALIGN_MAX_ROUNDS = 1024, 131072, 16      # GENIE_TMALIGN_MAX_LENGTH, _MAX_CELLS, _MAX_ROUNDS

FOLD_REPORT = ('tm_nearest', 'nearest', 'tm_lowest_wanted', 'n_fold_violations', 'e_fold')      # GENIE_FOLD_REPORT slots
FOLD_COUNTS = ('nearest', 'n_fold_violations')
FOLD_MAX_REFERENCES = 4096      # GENIE_FOLD_MAX_REFERENCES
FOLD_ALIGN_MAX_REFERENCES, FOLD_ALIGN_MAX_STRIDE = 1024, 64      # GENIE_FOLD_ALIGN_MAX_REFERENCES, _MAX_STRIDE
DIVERSITY_REPORT = ('tm_nearest_design', 'nearest_design', 'tm_mean_design', 'n_similar', 'e_diversity')      # GENIE_DIVERSITY_REPORT slots
DIVERSITY_COUNTS = ('nearest_design', 'n_similar')
DIVERSITY_MAX_BATCH = 1448      # GENIE_DIVERSITY_MAX_BATCH
BURIAL_REPORT = ('burial_mean', 'burial_min', 'burial_max', 'n_burial_violated', 'max_burial_violation', 'e_burial_target',
                 'e_burial_mean')      # GENIE_BURIAL_REPORT slots
BURIAL_COUNTS = ('n_burial_violated',)
BURIAL_MAX_LENGTH = 1728        # GENIE_BURIAL_MAX_LENGTH
ENVELOPE_REPORT = ('n_outside', 'max_outside', 'n_uncovered', 'max_uncovered', 'e_envelope_inside', 'e_envelope_cover')      # GENIE_ENVELOPE_REPORT slots
ENVELOPE_COUNTS = ('n_outside', 'n_uncovered')
ENVELOPE_EPS, ENVELOPE_CHUNK = 0.1, 1024        # GENIE_ENVELOPE_EPS, GENIE_ENVELOPE_CHUNK: the rows of the walked side staged in LDS at a time
ENVELOPE_FILL = 2048        # GENIE_ENVELOPE_FILL: work-groups of a launch from which it runs 4 waves per work-group instead of 16
ENVELOPE_MAX_LENGTH, ENVELOPE_MAX_POINTS = 4096, 16384      # GENIE_ENVELOPE_MAX_LENGTH, _MAX_POINTS
CONTEXT_REPORT = ('context_contacts', 'n_context_contacts', 'n_context_interface', 'context_min_distance', 'n_context_clash', 'anchor_rmsd',
                  'e_context_clash', 'e_context_contact')      # GENIE_CONTEXT_REPORT slots
CONTEXT_COUNTS = ('n_context_contacts', 'n_context_interface', 'n_context_clash')
CONTEXT_MAX_ATOMS = 12690       # GENIE_CONTEXT_MAX_ATOMS: the longest context whose staging fits in the kernel's 160 KiB of LDS
TMALIGN_NORMS = ('query', 'reference', 'shorter', 'longer')      # norm 0..3 of genie_tm_align and genie_fold_align_potential

_lib = None


class GenieError(RuntimeError):
    pass


def load_library():
    """dlopen the in-tree library and bind every declared entry point."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GenieError(
            f'{LIB_PATH} not found: build it with `python -m genie2_amd.build` '
            '(there is no CPU fallback for the denoising path)')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(handle, rc, what):
    if rc != 0:
        msg = load_library().genie_last_error(handle)
        raise GenieError(f'{what} failed (rc={rc}): {msg.decode() if msg else "?"}')
