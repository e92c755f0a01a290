/*
 * genie_hip.h -- C ABI of libgenie_hip.so: the MI355X (gfx950) denoising path
 * of Genie 2 (marvinli00/genie2), hand-written HIP behind plain pointers.
 *
 * The reference has no FFI of its own: its seam is the Python
 * call `self.model.model(ts, timesteps, features)['z']` inside the reverse
 * loop.  Each entry point below names the reference code it replaces
 * (paths relative to the reference root); genie_shape_potential,
 * genie_sheet_potential and genie_symmetry_potential, the shape, the
 * strand-pairing and the symmetry potential of guided sampling, have no
 * counterpart there and say so, and
 * genie_secstruct_potential has no differentiable one.
 *
 * Conventions
 *   - return 0 = ok, < 0 = error (GENIE_E_*); text via genie_last_error().
 *     No C++ exception crosses this boundary.
 *   - the caller owns every tensor buffer passed in (device memory on the
 *     handle's device unless marked HOST; contiguous; fp32 / int32 / uint8);
 *     the library owns the handle, packed weights, tables and workspace.
 *   - all device work is enqueued on the caller's stream and is asynchronous;
 *     no entry point except genie_create / genie_load_weights /
 *     genie_set_tables / genie_profile_read synchronises.
 *   - a handle is single-threaded: one per (process, device), matching the
 *     reference's one-process-per-device launcher
 *     (genie/utils/multiprocessor.py:84-96).
 */
#ifndef GENIE_HIP_H
#define GENIE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GENIE_OK            0
#define GENIE_E_ARG        -1   /* bad argument / unsupported shape */
#define GENIE_E_STATE      -2   /* call order (weights/tables/features missing) */
#define GENIE_E_HIP        -3   /* HIP runtime error */
#define GENIE_E_NOMEM      -4

typedef struct genie_ctx* genie_handle_t;
typedef void* genie_stream_t;           /* hipStream_t */

/* Mirrors the keys of Config.model / .diffusion / .io that
 * Denoiser(**config.model, n_timestep, max_n_res, max_n_chain) consumes
 * (genie/config.py:36-80, genie/diffusion/ddpm.py:26-31). */
typedef struct {
    int32_t c_s, c_p;
    int32_t c_pos_emb, c_chain_emb, c_timestep_emb;
    int32_t relpos_k;
    int32_t template_dist_n_bin;
    float   template_dist_min, template_dist_step;
    int32_t n_pair_transform_layer, c_hidden_mul, pair_transition_n;
    int32_t n_structure_layer, n_structure_block;
    int32_t c_hidden_ipa, n_head_ipa, n_qk_point, n_v_point;
    float   rescale;
    int32_t n_timestep, max_n_res, max_n_chain;
    /* triangular attention of the pair stack (include_tri_att; genie/model/pair_transform_net.py:69-79): per-head width and
     * number of heads.  n_head_tri == 0 (a zero-initialised tail): none, and c_hidden_tri_att is ignored.  Supported:
     * (c_hidden_tri_att, n_head_tri) = (32, 4) and (16, 8); genie_create refuses anything else. */
    int32_t c_hidden_tri_att, n_head_tri;
} genie_dims_t;

/* The tensors of the reference's 12-key feature dict the denoiser reads
 * (genie/utils/feat_utils.py:304-321; model/ *.py).  bool tensors are passed
 * as their 1-byte storage. */
typedef struct {
    const int32_t* aatype;               /* [B,N,20] */
    const float*   atom_positions;       /* [B,N,3]  motif coordinates */
    const int32_t* residue_mask;         /* [B,N]    */
    const int32_t* residue_index;        /* [B,N]    */
    const int32_t* chain_index;          /* [B,N]    */
    const uint8_t* fixed_sequence_mask;  /* [B,N]    */
    const uint8_t* fixed_structure_mask; /* [B,N,N]  */
    const uint8_t* interface_mask;       /* [B,N]    */
} genie_features_t;

/* Optional stage outputs of one denoiser call (any pointer may be NULL).
 * They are the other entries of the dict Denoiser.forward returns
 * (genie/model/model.py:186-192) plus two intermediate taps for tests. */
typedef struct {
    float* s;          /* [B,N,c_s]      's'  (single feature net output)      */
    float* p;          /* [B,N,N,c_p]    'p'  (pair transform net output)      */
    float* s_final;    /* [B,N,c_s]      'states'[-1]                          */
    float* rots_out;   /* [B,N,3,3]      'ts'.rots                             */
    float* trans_out;  /* [B,N,3]        'ts'.trans                            */
    float* p_init;     /* [B,N,N,c_p]    pair feature net output (test tap)    */
    float* p_layer0;   /* [B,N,N,c_p]    after pair transform layer 0 (tap)    */
    float* states;     /* [1+blocks*layers,B,N,c_s] 'states' (structure_net.py:236-243) */
    float* p_trimul_out0; /* [B,N,N,c_p] p after layer 0's outgoing triangle multiplication (pair_transform_net.py:109-110; tap) */
    float* ipa_cat0;   /* [B,N,H*(c_hidden+4*Pv+c_p)] input of layer 0's IPA linear_out (invariant_point_attention.py:251-258; tap) */
    float* p_tri_att0; /* [B,N,N,c_p] p after layer 0's ending-node triangular attention, before its pair transition
                          (pair_transform_net.py:113-115; tap; written only with n_head_tri > 0; padded pairs hold free, finite values) */
} genie_taps_t;

/* ---- lifetime ---------------------------------------------------------- */

/* Replaces Denoiser.__init__ (genie/model/model.py:20-123).  Unsupported dims are refused with GENIE_E_ARG before the device is
 * touched; genie_last_error(NULL) names the field. */
int genie_create(const genie_dims_t* dims, int device, genie_handle_t* out);
void genie_destroy(genie_handle_t h);
const char* genie_last_error(genie_handle_t h);   /* h may be NULL: last error of genie_create or of an entry that takes no handle */

/* Number of fp32 values genie_load_weights expects for these dims. */
size_t genie_weight_count(const genie_dims_t* dims);

/* Replaces load_state_dict: `blob` (HOST) is every tensor of
 * Denoiser.state_dict() in its own order (checkpoint
 * keys are these with a 'model.' prefix, genie/utils/model_io.py:159-173),
 * each [out,in] row-major, concatenated.  Repacked into MFMA fragment order
 * and uploaded.  With n_head_tri > 0 the tensors of tri_att_start and tri_att_end
 * sit between tri_mul_in.* and pair_transition.* of every layer, as in the reference. */
int genie_load_weights(genie_handle_t h, const float* blob, size_t n_floats);

/* Sinusoidal tables and the diffusion schedule, computed by the host with
 * the reference's own expressions (genie/utils/encoding.py:5-25,
 * genie/diffusion/ddpm.py:40-56) and uploaded once.  All HOST pointers.
 *   pos_tab   [n_pos][c_pos_emb]      row v = encoding of residue_index v
 *   chain_tab [n_chain][c_chain_emb]  row v = encoding of chain_index v
 *   t_tab     [n_timestep+1][c_timestep_emb]
 *   sched     [4][n_timestep+1] = alphas, sqrt_alphas,
 *             sqrt_one_minus_alphas_cumprod, sqrt_betas */
int genie_set_tables(genie_handle_t h, const float* pos_tab, int n_pos,
                     const float* chain_tab, int n_chain,
                     const float* t_tab, const float* sched);

/* ---- per batch --------------------------------------------------------- */

/* Binds a batch of features (device pointers are read now and copied into
 * library-owned buffers) and computes the step-invariant pair terms
 * (_relpos and the motif template: genie/model/pair_feature_net.py:134,
 * 149-158,166-221).  Sizes the workspace for (B, N). */
int genie_prepare_features(genie_handle_t h, genie_stream_t stream, int B, int N,
                           const genie_features_t* feats);

/* compute_frenet_frames (genie/utils/geo_utils.py:21-85) for the bound batch. */
int genie_frenet(genie_handle_t h, genie_stream_t stream, const float* trans /*[B,N,3]*/,
                 float* rots_out /*[B,N,3,3]*/);

/* The same without a handle, as the reference's callers use it: compute_frenet_frames(coords, chains, mask)
 * (genie/utils/geo_utils.py:21; callers sampler/base.py:228,282, diffusion/genie.py:86).  chains / mask: int32 [B,N]. */
int genie_frenet_frames(genie_stream_t stream, int B, int N, const float* coords /*[B,N,3]*/, const int32_t* chains,
                        const int32_t* mask, float* rots_out /*[B,N,3,3]*/);

/* The motif potential of twisted-diffusion / SMC sampling with its gradient, without a handle: the fork's motif twisting function
 * (genie/sampler/unconditional_smc.py:303-345; genie2_amd/smc.py:58-69 restates it in PyTorch), one pass over every placement
 * instead of a Python loop and an autograd walk back through it.  Placement p puts segment s at residues
 * starts[p,s] .. starts[p,s] + seg_len[s] - 1 (in order, without overlap, inside 0..N-1: the caller validates `starts` once when it
 * builds it); motif position m runs over the segments in order, as x0[:, mask] selects.  With M = sum seg_len:
 *   c_bp(m) = x0[b, r_p(m)] - mean_m x0[b, r_p(m)],   e_bp(m) = c_bp(m) - target[m]
 *   score[b,p] = -sum_m |e_bp(m)|^2 / (2 var),        logp_out[b] = logsumexp_p score[b,p] - log P
 *   grad_out[b,n] = d logp[b] / d x0[b,n] = -sum_p w_bp [n in p] (e_bp(m_p(n)) - mean_m e_bp(m)) / var,  w_bp = softmax_p score[b,:]
 * (exactly 0 at residues no placement covers).  `var` is one float in device memory (the sampler computes it on the device).
 * seg_len, starts, target: device int32 [S], int32 [P,S], f32 [M,3].  One launch, or two when P is large enough that the placement
 * scores spill to `work` (genie_motif_potential_work_bytes(B, P) bytes, 16-byte aligned; 0 = none needed, `work` may be NULL).
 * No allocation, no synchronisation; bitwise reproducible (no atomics: the gradient is gathered per residue in a fixed order).
 * Returns 0, or -1 for an impossible shape (P, S or M < 1, M > N, too little work) or a problem that does not fit in LDS. */
int genie_motif_potential(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/, int P, int S, int M,
                          const int32_t* seg_len /*[S]*/, const int32_t* starts /*[P,S]*/, const float* target /*[M,3]*/,
                          const float* var /*[1], device*/, float* logp_out /*[B]*/, float* grad_out /*[B,N,3]*/, void* work,
                          size_t work_bytes);
size_t genie_motif_potential_work_bytes(int B, int P);

/* The same potential after optimal superposition: every placement is compared to the motif in its best-fitting orientation, not in
 * the one the motif file happens to be written in.  With t_c = target - mean(target) and c_bp as above:
 *   R_bp = argmin over proper rotations (det +1) of sum_m |c_bp(m) - R t_c(m)|^2     (Horn's quaternion, float32 Jacobi sweeps)
 *   e_bp(m) = c_bp(m) - R_bp t_c(m),   q_bp = sum_m |e_bp(m)|^2   (summed from the residuals, not from the eigenvalue)
 *   score[b,p] = -q_bp / (2 var),      logp_out[b] = logsumexp_p score[b,p] - log P
 *   grad_out[b,n] = -sum_p w_bp [n in p] e_bp(m_p(n)) / var,  w_bp = softmax_p score[b,:]
 * (the derivative through R vanishes at the optimum and sum_m e = 0; exactly 0 at residues no placement covers).
 *   best_out[b] = the lowest p with the largest score,   rmsd_out[b] = sqrt(q_{b,best} / M): the superposed motif RMSD.
 * A mirror image does not fit (R is proper); a collinear selection has no unique R but a unique score, and every output stays finite.
 * logp_out and grad_out are given together or both NULL; best_out and rmsd_out may each be NULL; at least one output is asked for.
 * Arguments, `work` (genie_motif_potential_rigid_work_bytes(B, P) bytes, 16-byte aligned; 0 = none needed), launches (one, or two when
 * the placement records spill), reproducibility and the return value are as for genie_motif_potential; M < 3 is refused too. */
int genie_motif_potential_rigid(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/, int P, int S, int M,
                                const int32_t* seg_len /*[S]*/, const int32_t* starts /*[P,S]*/, const float* target /*[M,3]*/,
                                const float* var /*[1], device*/, float* logp_out /*[B] or NULL*/, float* grad_out /*[B,N,3] or NULL*/,
                                int32_t* best_out /*[B] or NULL*/, float* rmsd_out /*[B] or NULL*/, void* work, size_t work_bytes);
size_t genie_motif_potential_rigid_work_bytes(int B, int P);

/* The same potential for a multi-motif problem: segment s belongs to motif group seg_group[s] in 0..G-1 (every group non-empty,
 * numbered by first appearance in segment order; a group's segments need not be adjacent).  The segments of one group keep their
 * relative pose; different groups are independent bodies, so every group is compared on its own, translated (align 0) or superposed
 * (align 1).  Placements stay joint: all segments in order, without overlap, one softmax over p.  For group g with M_g residues,
 * m running over its motif positions:
 *   c^g_bp(m) = x0[b, r_p(m)] - mean_{m in g} x0[b, r_p(m)],   t^g(m) = target[m] - mean_{m in g} target[m]   (centred here, per group)
 *   e^g_bp(m) = c^g_bp(m) - R^g_bp t^g(m),   R^g = I (align 0) or argmin over proper rotations of sum_{m in g} |c^g - R t^g|^2 (align 1)
 *   q^g_bp = sum_{m in g} |e^g_bp(m)|^2 (from the residuals),   q_bp = sum_g q^g_bp,   score[b,p] = -q_bp / (2 var)
 *   logp_out[b] = logsumexp_p score[b,p] - log P,   grad_out[b,n] = -sum_p w_bp [n in p] e^{g(n)}_bp(m_p(n)) / var,  w = softmax_p score
 * (exactly 0 at residues no placement covers),
 *   best_out[b] = the lowest p with the largest score,   rmsd_out[b] = sqrt(q_{b,best} / M),
 *   group_rmsd_out[b,g] = sqrt(q^g_{b,best} / M_g): every group's own RMSD in that placement.
 * With G = 1 this is genie_motif_potential (of a centred target) or genie_motif_potential_rigid, to rounding.
 * logp_out and grad_out are given together or both NULL; best_out, rmsd_out, group_rmsd_out may each be NULL; at least one output is
 * asked for; without a gradient one work-group per particle runs.  A placement's record is per group (16 B per group, 32 B with a
 * rotation, plus 4 B per placement): records stay in LDS up to 96 KiB of them -- 1445 placements of 2 superposed groups, 378 of
 * GENIE_MOTIF_MAX_GROUPS -- and spill to `work` beyond (genie_motif_potential_grouped_work_bytes(B, P, G, align) bytes, 16-byte
 * aligned; 0 = none needed), with a second launch.  No allocation, no synchronisation, bitwise reproducible, as above.
 * Returns -1, before the device is touched, for G < 1, G > GENIE_MOTIF_MAX_GROUPS, G > S, align not 0 or 1, M < 3 G with align 1
 * (every group needs 3 residues to be superposed: seg_len is device memory, so the caller checks the groups themselves), and for
 * what genie_motif_potential_rigid refuses. */
#define GENIE_MOTIF_MAX_GROUPS 8
int genie_motif_potential_grouped(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/, int P, int S, int M, int G,
                                  const int32_t* seg_len /*[S]*/, const int32_t* seg_group /*[S]*/, const int32_t* starts /*[P,S]*/,
                                  const float* target /*[M,3]*/, const float* var /*[1], device*/, int align /*0 translation, 1 rigid*/,
                                  float* logp_out /*[B] or NULL*/, float* grad_out /*[B,N,3] or NULL*/, int32_t* best_out /*[B] or NULL*/,
                                  float* rmsd_out /*[B] or NULL*/, float* group_rmsd_out /*[B,G] or NULL*/, void* work,
                                  size_t work_bytes);
size_t genie_motif_potential_grouped_work_bytes(int B, int P, int G, int align);

/* The SMC bookkeeping of one twisted step for S independent particle systems of K particles each, without a handle: the fork's weight
 * helpers, systematic resampling and the weight update of its loop (genie/sampler/unconditional_smc.py:25-43, 237-288, 540-576;
 * genie2_amd/smc.py:212-226 restates them in PyTorch for one system).  Layout is system-major: particle b belongs to system b / K.
 * For every system s on its own, over its K particles:
 *   d_b     = sum_{n,c} [ (x_new - mean_tw)^2 - (x_new - mean_un)^2 ] / (2 sigma^2)   (= log_rev - log_tw: the log sigma terms cancel)
 *   log_w_b = d_b + log_prob_b - log_proposal_b + log_w_acc_b
 *   ess_s   = (sum w)^2 / sum w^2,  w = softmax of log_w over the system
 *   if ess_s < ess_fraction K:  systematic resampling with the points u_s + i / K, i = 0..K-1: the ancestor of particle i is the
 *       number of cumulative sums of w strictly below its point, clamped into the system;
 *       x_out[b] = x_new[ancestor],  log_proposal[b] = log_prob[ancestor],  log_w_acc[b] = 0
 *   else:  x_out = x_new,  log_proposal = log_prob,  log_w_acc = log_w - logsumexp_s(log_w) + log K
 * All N rows are summed (the twisted sampler's batches are never ragged).  index_out[b] is the ancestor as a batch index (b itself
 * where the system did not resample), ess_out[s] the effective sample size, resampled_out[s] 1 or 0.  A particle whose log_w is -inf
 * has weight exactly 0 and is never an ancestor (the clamp is to the first and last particle of non-zero weight).  A system whose
 * largest log_w is not finite (a NaN counts) is left in place: identity indices, resampled_out 0, log_w_acc as the formula gives it.
 * Two launches on `stream`: the first sums d_b, one work-group per particle, and writes log_w_b to `work` (a double per particle:
 * genie_smc_reweight_work_bytes(S, K, N) bytes, 8-byte aligned); the second copies x_out, every work-group redoing its system's
 * K-value tail in one wave.  The sums of d_b and the whole tail (softmax, ESS, cumulative sums, the comparison with the points) run
 * in float64, in a fixed order, without atomics: two calls on the same inputs give bitwise the same outputs.  No allocation, no
 * synchronisation, no host read.
 * Returns GENIE_E_ARG, before anything is launched, with genie_last_error(NULL) naming this entry: a NULL pointer; K outside 1..64;
 * S < 1; N < 1; x_out overlapping x_new; log_proposal overlapping log_prob; a non-finite ess_fraction; work_bytes below
 * genie_smc_reweight_work_bytes(S, K, N). */
int genie_smc_reweight(genie_stream_t stream, int S, int K, int N, const float* x_new /*[S K,N,3]*/, const float* mean_tw /*[S K,N,3]*/,
                       const float* mean_un /*[S K,N,3]*/, const float* sigma /*[1], device*/, const float* log_prob /*[S K]*/,
                       const float* u /*[S], each in [0, 1/K)*/, double ess_fraction, float* log_proposal /*[S K], in/out*/,
                       float* log_w_acc /*[S K], in/out*/, float* x_out /*[S K,N,3]*/, int32_t* index_out /*[S K]*/,
                       float* ess_out /*[S]*/, int32_t* resampled_out /*[S]*/, void* work, size_t work_bytes);
size_t genie_smc_reweight_work_bytes(int S, int K, int N);

/* The shape potential of twisted-diffusion / SMC sampling with its gradient and a per-particle report, without a handle: a
 * radius-of-gyration cap, a C-alpha clash term over all residue pairs and the caller's pairwise distance restraints
 * (csrc/shape_kernels.hip; the reference has no counterpart, its one twisting function is the motif potential above).  For particle b
 * with coordinates x_n (n = 0..N-1, Angstrom); all N rows are used (the twisted sampler's batches are never ragged):
 *   centroid  m = mean_n x_n,  c_n = x_n - m,  rog = sqrt(sum_n |c_n|^2 / N)
 *   E_rog   = rog_weight   * max(0, rog - rog_max)^2
 *   E_clash = clash_weight * sum_{i<j, j-i >= clash_separation} max(0, clash_distance - d_ij)^2,   d_ij = |x_i - x_j|
 *   E_rst   = sum_r w_r * ( max(0, lo_r - d_r)^2 + max(0, d_r - hi_r)^2 ),   d_r = |x_{i_r} - x_{j_r}|   (hi_r may be +inf, lo_r may be 0)
 *   logp_out[b] = -(E_rog + E_clash + E_rst) / (2 var)
 *   grad_out[b,n] = d logp[b] / d x_n
 *                 = -(1/var) * [ rog_weight (rog - rog_max)_+ c_n / (N rog)
 *                                - clash_weight sum_{j eligible} (clash_distance - d_nj)_+ u_nj
 *                                + sum_{r containing n} w_r ((d_r - hi_r)_+ - (lo_r - d_r)_+) u_{n,partner} ],      u_nj = (x_n - x_j) / d_nj
 * Where a distance, or rog, is exactly 0 in float32 its direction is 0: every output stays finite.  `var` is one float in device
 * memory.  The likelihood is left unnormalised: every use in the sampler is a difference or a normalised weight.
 * Restraints arrive as a per-residue table the host builds once (device memory): the entries of residue n are
 * rst_offset[n] .. rst_offset[n+1] - 1 (rst_offset[0] = 0, rst_offset[N] = R2), entry k naming the partner rst_partner[k] and the
 * restraint's lo, hi and weight.  Every restraint is listed at both of its residues (R2 = twice their number), partners ascending
 * within a residue, so a residue's force is a gather in a fixed order; energies and counts are taken from the entries with
 * partner > residue.  R2 = 0: no restraints, the five pointers may be NULL.  The caller validates the table; offsets and partners are
 * clamped into range all the same.
 * rog_weight == 0 or clash_weight == 0 switches that term off (energy and force).  report_out[b] holds GENIE_SHAPE_REPORT floats:
 *   rog, min_distance, n_clash, e_rog, e_clash, e_restraint, n_violated, max_violation
 * min_distance and n_clash (pairs with d < clash_distance) are always taken over the eligible pairs, whatever the weight, and
 * min_distance is +inf when there is none; n_violated counts the restraints with d < lo or d > hi and max_violation is the largest
 * such excess in Angstrom (0 when none); the three energies are the weighted E above, before the division by 2 var.  (Counts are
 * stored as floats: exact up to 2^24.)
 * logp_out and grad_out are given together or both NULL; report_out may be NULL; at least one output is asked for.
 * Two launches on `stream`: grid (ceil(N / 64), B) work-groups that stage x0[b] in LDS (12 N bytes) and leave 8 partial values per
 * tile in `work` (genie_shape_potential_work_bytes(B, N) = B * ceil(N / 64) * 32 bytes, 4-byte aligned), then one thread per
 * particle that adds them in tile order.  No allocation, no synchronisation, no host read, no atomics: every output is written once
 * in a fixed order, so two calls on the same inputs are bitwise equal.
 * Returns GENIE_E_ARG, before the device is touched, with genie_last_error(NULL) naming this entry and the argument: B < 1 (or above
 * 65535); N < 1; x0 or var NULL; no output asked for; logp_out and grad_out not given together; clash_separation < 1; a negative or
 * non-finite rog_max, clash_distance, rog_weight or clash_weight; R2 < 0, R2 odd, or R2 > 0 with a NULL table; `work` NULL,
 * misaligned or work_bytes too small; an N whose staging does not fit in LDS (160 KiB: N above 13 140). */
#define GENIE_SHAPE_REPORT 8   /* rog, min_distance, n_clash, e_rog, e_clash, e_restraint, n_violated, max_violation */
int genie_shape_potential(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/,
                          float rog_max, float rog_weight, float clash_distance, int clash_separation, float clash_weight,
                          int R2, const int32_t* rst_offset /*[N+1]*/, const int32_t* rst_partner /*[R2]*/, const float* rst_lo,
                          const float* rst_hi, const float* rst_weight /*[R2] each*/, const float* var /*[1], device*/,
                          float* logp_out /*[B] or NULL*/, float* grad_out /*[B,N,3] or NULL*/,
                          float* report_out /*[B,GENIE_SHAPE_REPORT] or NULL*/, void* work, size_t work_bytes);
size_t genie_shape_potential_work_bytes(int B, int N);

/* The secondary-structure potential of twisted-diffusion / SMC sampling with its gradient, a per-particle report and a hard
 * assignment, without a handle: soft bounds on the helix and the extended content and an optional per-residue blueprint, scored on
 * C-alpha geometry alone (csrc/secstruct_kernels.hip).  The reference has no differentiable counterpart: the example statistic of
 * genie/sampler/secstruct.py ("more than 50 % alpha-helix") writes a PDB and runs biotite's P-SEA assignment on the host.  For
 * particle b with coordinates x_n (n = 0..N-1, Angstrom; all N rows are used) there are W = N - 4 windows, window i covering
 * residues i..i+4, with four features
 *   d2 = |x_{i+2} - x_i|,  d3 = |x_{i+3} - x_i|,  d4 = |x_{i+4} - x_i|,
 *   chi = ((b1 x b2) . b3) / (|b1| |b2| |b3|),   b_k = x_{i+k} - x_{i+k-1}, k = 1..3
 * (chi is smooth, lies in [-1, 1] and changes sign under mirroring, which distances cannot).  For class c in {H (helix), E
 * (extended)} `table` holds four targets mu and four tolerances sigma, 16 host floats copied by value: H mu[4], H sigma[4], E mu[4],
 * E sigma[4], each in the order d2, d3, d4, chi.  Per window
 *   z_cf = (f - mu_cf) / sigma_cf,   u_c,i = 1/4 sum_f z_cf^2,   s_c,i = 1 / (1 + u_c,i)
 * (a rational score: its gradient decays polynomially, so a coil far from any target is still guided, and it needs no exp), and
 * with the soft window count n_c = sum_i s_c,i
 *   E_c   = c_weight * [ max(0, W c_min - n_c)^2 + max(0, n_c - W c_max)^2 ]      c = helix, extended; the bounds are fractions
 *   E_tgt = target_weight * sum_{i targeted as c} u_c,i
 *   logp_out[b] = -(E_H + E_E + E_tgt) / (2 var)
 *   grad_out[b,n] = d logp[b] / d x_n, analytic, with d s / d x = -s^2 d u / d x
 * Counts, not fractions, enter the hinge, so the force per window does not shrink with N.  `target` is N int8 codes in device
 * memory, 0 free, 1 H, 2 E (any other value counts as 0), or NULL: window i is targeted as c when target[i..i+4] all equal c.
 * A distance that is exactly 0 in float32 has direction 0, and a window with any |b_k| = 0 has chi = 0 and no chi force: every
 * output is finite for finite inputs.  A weight of 0 switches its term off (energy and force).  `var` is one float in device memory;
 * the likelihood is left unnormalised.
 * Hard assignment (for reporting, not differentiated): window i is class c when all four |z_cf| <= 1; residue n is H if any window
 * containing it is H, otherwise E if any is E, otherwise C.  assign_out[b,n] is 0 C, 1 H, 2 E.  "Extended" is local geometry only:
 * there is no strand pairing (genie_sheet_potential, below, scores it).  report_out[b] holds GENIE_SECSTRUCT_REPORT floats:
 *   helix_content (n_H / W), extended_content (n_E / W), n_helix, n_extended (residues of the hard assignment), e_helix, e_extended,
 *   e_target (the weighted E above, before the division by 2 var), n_target_missed (residues with target H or E whose hard
 *   assignment differs; 0 with a NULL target)
 * (counts are stored as floats: exact up to 2^24).  logp_out and grad_out are given together or both NULL; report_out and assign_out
 * may be NULL; at least one output is asked for.
 * One launch on `stream`: one work-group of 256 threads per particle stages x0[b] and its windows in LDS (32 N bytes), reduces in a
 * fixed tree and computes the gradient as a gather over the at most five windows of a residue.  No allocation, no synchronisation,
 * no host read, no atomics, no work buffer: every output is written once in a fixed order, so two calls on the same inputs are
 * bitwise equal.
 * Returns GENIE_E_ARG, before the device is touched, with genie_last_error(NULL) naming this entry and the argument: B < 1 (or above
 * 65535); N < 5; x0, var or table NULL; no output asked for; logp_out and grad_out not given together; a sigma that is <= 0 or not
 * finite (or a mu that is not finite); a negative or non-finite weight; a bound outside [0, 1] or min > max; target_weight > 0 with
 * a NULL target; an N whose staging does not fit in LDS (160 KiB: N above 5 122). */
#define GENIE_SECSTRUCT_REPORT 8   /* helix_content, extended_content, n_helix, n_extended, e_helix, e_extended, e_target, n_target_missed */
int genie_secstruct_potential(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/,
                              const float* table /*16 host floats: H mu[4], H sigma[4], E mu[4], E sigma[4]*/,
                              float helix_min, float helix_max, float helix_weight,
                              float extended_min, float extended_max, float extended_weight,
                              const int8_t* target /*[N] device, or NULL*/, float target_weight,
                              const float* var /*[1], device*/, float* logp_out /*[B] or NULL*/, float* grad_out /*[B,N,3] or NULL*/,
                              float* report_out /*[B,GENIE_SECSTRUCT_REPORT] or NULL*/, int8_t* assign_out /*[B,N] or NULL; 0 C, 1 H, 2 E*/);

/* The sheet potential of twisted-diffusion / SMC sampling with its gradient, a per-particle report and every residue's pairing
 * partner, without a handle: soft bounds on the antiparallel and the parallel strand-pairing content and an optional ladder of
 * listed rungs, scored on C-alpha distances alone (csrc/sheet_kernels.hip).  It is what genie_secstruct_potential's "extended" class
 * leaves out; the reference has no counterpart.  For particle b with coordinates x_n (n = 0..N-1, Angstrom; all N rows are used)
 * and class c in {A (antiparallel), P (parallel)} a rung is a pair (i, j) of interior residues, 1 <= i < j <= N-2, j - i >= sep_c,
 * with three distances
 *   A: d0 = |x_i - x_j|,  d1 = |x_{i-1} - x_{j+1}|,  d2 = |x_{i+1} - x_{j-1}|
 *   P: d0 = |x_i - x_j|,  d1 = |x_{i-1} - x_{j-1}|,  d2 = |x_{i+1} - x_{j+1}|
 * (the neighbours of a paired residue are paired with the neighbours of its partner, in the opposite or in the same direction).
 * Four floats passed by value hold a target and a tolerance per class: mu_A = 5.0, sigma_A = 0.6, mu_P = 4.8, sigma_P = 0.5 A are the
 * defaults the Python layer passes.  Per rung
 *   z_f = (d_f - mu_c) / sigma_c,   u_c,ij = 1/3 sum_f z_f^2,   s_c,ij = 1 / (1 + u_c,ij)^2,   n_c = sum_rungs s_c,ij
 * (squared-rational: the plain 1 / (1 + u) of the secondary-structure potential decays so slowly that the far pairs of a compact
 * chain add up to more than the signal of a sheet; this one still needs no exp), and with the soft rung count n_c
 *   E_c   = c_weight * [ max(0, N c_min - n_c)^2 + max(0, n_c - N c_max)^2 ]       c = antiparallel, parallel
 *   E_lad = ladder_weight * sum_r w_r u_{c_r}(i_r, j_r)                            over the listed rungs r = (i_r, j_r, c_r, w_r)
 *   logp_out[b] = -(E_A + E_P + E_lad) / (2 var)
 *   grad_out[b,n] = d logp[b] / d x_n, analytic, with d s / d u = -2 / (1 + u)^3 and d u / d d_f = 2 z_f / (3 sigma_c)
 * The bounds are in rungs per residue (an interior strand of a large sheet approaches 1); c_max = +inf is no upper bound.  Counts,
 * not fractions, enter the hinge.  A distance that is exactly 0 in float32 has direction 0: every output is finite for finite
 * inputs.  A weight of 0 switches its term off (energy and force).  `var` is one float in device memory; the likelihood is left
 * unnormalised.  N < 6 has no eligible rung: n_c = 0, logp from the hinges alone, a gradient of 0 and every partner -1.
 * The ladder arrives as a per-residue table of harmonic distance terms the host builds once (device memory), since u is a sum of
 * three squared distance deviations: E_lad = ladder_weight * sum_terms coef (|x_p - x_q| - mu)^2, coef = w_r / (3 sigma_c^2), the
 * coefficients of a distance that neighbouring rungs of one class share merged.  The entries of residue n are lad_offset[n] ..
 * lad_offset[n+1] - 1 (lad_offset[0] = 0, lad_offset[N] = L2), entry k naming the partner in the low bits of lad_partner[k], its mu
 * and coef.  Every term is listed at both of its residues (L2 = twice their number), partners ascending within a residue, so a
 * residue's force is a gather in a fixed order; energies are taken from the entries with partner > residue.  lad_partner[k] also
 * carries GENIE_SHEET_PARALLEL where the term belongs to class P and GENIE_SHEET_RUNG where it is the d0 of a listed rung (those
 * entries are what n_ladder_missed counts).  L2 = 0: no ladder, the four pointers may be NULL.  The caller validates the table;
 * offsets and partners are clamped into range all the same.
 * Hard assignment (for reporting, not differentiated): a rung is formed in class c when all three |z_f| <= 1; a residue is paired
 * when it is the i or the j of a formed rung.  pairs_out[b,n,0] is the partner of residue n's formed antiparallel rung with the
 * highest s, pairs_out[b,n,1] the same for parallel; -1: none; of equal s the lowest partner.  report_out[b] holds
 * GENIE_SHEET_REPORT floats:
 *   antiparallel_content (n_A / N), parallel_content (n_P / N), n_antiparallel, n_parallel (formed rungs), n_paired (paired
 *   residues), e_antiparallel, e_parallel, e_ladder (the weighted E above, before the division by 2 var), n_ladder_missed (listed
 *   rungs that are not formed in their class, whatever their separation; 0 without a ladder)
 * (counts are stored as floats: exact up to 2^24).  logp_out and grad_out are given together or both NULL; report_out and pairs_out
 * may be NULL; at least one output is asked for.
 * Two launches on `stream`: grid (ceil(N / 64), B) work-groups that stage x0[b] in LDS (12 N + 14 336 bytes), walk all partners of
 * their 64 residues as a gather (a rung's force lands on six residues: each lane recomputes, per partner, the up to six rungs that
 * hold that distance from nine distances, and no lane writes another lane's residue) and leave three unscaled gradient fields and 8
 * partial values per tile in `work` (genie_sheet_potential_work_bytes(B, N) = B * (36 N + 32 ceil(N / 64)) bytes, 4-byte aligned);
 * then the same grid with 64 threads adds the tiles in tile order, forms the hinge coefficients, which depend on the particle-wide
 * n_c, and writes the gradient, logp and the report.  With both class weights 0 and neither report nor pairs asked for the pair walk
 * is skipped.  No allocation, no synchronisation, no host read, no atomics: every output is written once in a fixed order, so two
 * calls on the same inputs are bitwise equal.
 * Returns GENIE_E_ARG, before the device is touched, with genie_last_error(NULL) naming this entry and the argument: B < 1 (or above
 * 65535); N < 1; x0 or var NULL; no output asked for; logp_out and grad_out not given together; a separation below 3; a sigma that is
 * <= 0 or not finite (or a mu that is not finite); a negative or non-finite weight; a bound that is negative or NaN, an infinite
 * minimum, or min > max; L2 < 0, L2 odd, or L2 > 0 with a NULL table; `work` NULL, misaligned or work_bytes too small; an N whose
 * staging does not fit in LDS (160 KiB: N above 12 458). */
#define GENIE_SHEET_REPORT 9   /* antiparallel_content, parallel_content, n_antiparallel, n_parallel, n_paired, e_antiparallel,
                                  e_parallel, e_ladder, n_ladder_missed */
#define GENIE_SHEET_PARALLEL (1 << 29)   /* lad_partner flag: the term belongs to class P */
#define GENIE_SHEET_RUNG (1 << 30)       /* lad_partner flag: the term is the d0 of a listed rung */
int genie_sheet_potential(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/,
                          float mu_antiparallel, float sigma_antiparallel, float mu_parallel, float sigma_parallel,
                          int separation_antiparallel, int separation_parallel,
                          float antiparallel_min, float antiparallel_max, float antiparallel_weight,
                          float parallel_min, float parallel_max, float parallel_weight,
                          int L2, const int32_t* lad_offset /*[N+1]*/, const int32_t* lad_partner /*[L2]*/, const float* lad_mu,
                          const float* lad_coef /*[L2] each*/, float ladder_weight, const float* var /*[1], device*/,
                          float* logp_out /*[B] or NULL*/, float* grad_out /*[B,N,3] or NULL*/,
                          float* report_out /*[B,GENIE_SHEET_REPORT] or NULL*/, int32_t* pairs_out /*[B,N,2] or NULL; -1: none*/,
                          void* work, size_t work_bytes);
size_t genie_sheet_potential_work_bytes(int B, int N);

/* The symmetry potential of twisted-diffusion / SMC sampling with its gradient and a per-particle report, without a handle: how far a
 * chain is from repeating itself under one or two generators (csrc/symmetry_kernels.hip).  It is what the other potentials, which all
 * act inside one asymmetric chain, cannot ask for: a cyclic or dihedral oligomer, a closed toroid of identical units, an open repeat
 * whose units follow one another by one screw motion.  The reference has no counterpart.
 * Layout (what the Python layer builds; the entry itself only sees generators): U units of m residues, unit k starting at
 * offset + k (m + linker), residue (k, a) = start_k + a, offset + U m + (U - 1) linker <= N; residues in no unit are free, and the
 * gradient there is exactly 0.  A generator is a list of L >= 3 pairs (src_i, dst_i) of distinct residues, no residue a source twice
 * and none a destination twice within one generator; at most GENIE_SYMMETRY_MAX_GENERATORS of them:
 *   C<n>, U = n:   g0: (k, a) -> ((k + 1) mod n, a), L = n m
 *   D<n>, U = 2n:  units 0..n-1 one ring, n..2n-1 the other; g0 (the n-fold): (k, a) -> ((k + 1) mod n, a) for k < n and
 *                  (n + k, a) -> (n + (k - 1) mod n, a); g1 (the two-fold): (k, a) <-> (n + k, a) in both directions; L = 2 n m each
 *                  (as permutations g1 g0 g1 = g0^-1 and g0^n = id)
 *   R<n>, U = n:   g0: (k, a) -> (k + 1, a), k = 0..n-2, L = (n - 1) m: one rigid motion, a screw, carries units 0..n-2 onto 1..n-1
 * For particle b with coordinates x (Angstrom) and generator g
 *   c_s = mean_i x[src_i],  c_d = mean_i x[dst_i],  p_i = x[src_i] - c_s,  q_i = x[dst_i] - c_d
 *   R_g = argmin over proper rotations of sum_i |q_i - R p_i|^2: Horn's quaternion of the correlation sum_i p_i q_i^T (csrc/horn.h, as
 *         the rigid motif alignment finds it; a proper rotation, so a mirror image does not fit)
 *   E_g = sum_i |q_i - R_g p_i|^2, summed from the residuals, never as sum |q|^2 + sum |p|^2 - 2 lambda_max: near symmetry that
 *         difference of large numbers has no digits left
 *   logp_out[b] = -(weight0 E_0 + weight1 E_1) / (2 var)
 *   grad_out[b] = d logp[b] / d x, analytic, with R_g held at its optimum (to first order E does not move with R, and the residuals
 *         sum to 0, so the centroids drop out):  dE_g / dx[dst_i] += 2 (q_i - R_g p_i),  dE_g / dx[src_i] += -2 R_g^T (q_i - R_g p_i)
 * `var` is one float in device memory; the likelihood is left unnormalised.  A weight of 0 switches its generator off (energy and
 * force; the report still describes it).  The generators arrive as one per-residue table in device memory, partner int32 [G, 2, N]:
 * partner[g][0][i] is the residue i maps to as a source, partner[g][1][i] the residue that maps to i, -1 for none.  The caller
 * validates it (each row the inverse of the other); entries index LDS, so the kernel clamps them into 0..N-1 all the same.
 * report_out[b] holds GENIE_SYMMETRY_REPORT floats:
 *   e_symmetry (weight0 E_0 + weight1 E_1, before the division by 2 var), symmetry_rmsd (sqrt(sum_g E_g / sum_g L_g), unweighted),
 *   then per generator slot g = 0, 1: rmsd_g (sqrt(E_g / L_g)), angle_g (the rotation angle of R_g in degrees, in [0, 180], as
 *   2 atan2(|v|, |w|) of the quaternion (w, v): a two-fold has a symmetric correlation and sits at exactly 180 or 0, where acos has no
 *   digits), rise_g (|u_g . (c_d - R_g c_s)| in Angstrom, u_g the rotation axis; |c_d - R_g c_s| when the angle is 0; R_g fixes u_g, so
 *   it is evaluated as |u_g . (c_d - c_s)|)
 * an unused slot reports zeros.  For a closed C_n the angle tends to 360 / n and the rise to 0; for a repeat they are its twist and
 * rise.  Coincident or collinear residues have a degenerate largest eigenvalue: every output stays finite, E_g is still the minimum,
 * the rotation (angle, rise, gradient) is one of the equally good ones.  logp_out and grad_out are given together or both NULL;
 * report_out may be NULL; at least one output is asked for.
 * One launch on `stream`: grid B, 256 threads; the work-group of particle b stages x0[b] in LDS (12 N + 320 bytes) and makes three
 * passes over the residues, both generators in each: the centroids (c_d as c_s plus the mean of x[dst] - x[src]), the correlation,
 * then -- after wave g has solved the 4x4 eigenproblem of generator g, wave-uniform work -- the residuals, E_g and the gradient of
 * every residue as a gather through the table (a residue has at most one source and one destination role per generator).  Every sum
 * is a butterfly inside a wave and the four wave results in wave order.  No allocation, no synchronisation, no host read, no
 * atomics, no scatter: two calls on the same inputs are bitwise equal.  Nothing passes through memory between the passes, so
 * genie_symmetry_potential_work_bytes(B, N) is 0 and `work` may be NULL; the pair is taken so that every potential is called alike.
 * Returns GENIE_E_ARG, before the device is touched, with genie_last_error(NULL) naming this entry and the argument: B < 1 (or above
 * 65535); N < 1; x0, partner or var NULL; G outside 1..2; a negative or non-finite weight; no output asked for; logp_out and
 * grad_out not given together; `work` NULL with work_bytes above 0; an N whose staging does not fit in LDS (160 KiB: N above 13 626). */
#define GENIE_SYMMETRY_REPORT 8   /* e_symmetry, symmetry_rmsd, rmsd_0, angle_0, rise_0, rmsd_1, angle_1, rise_1 */
#define GENIE_SYMMETRY_MAX_GENERATORS 2
int genie_symmetry_potential(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/, int G,
                             const int32_t* partner /*[G,2,N], device*/, float weight0, float weight1,
                             const float* var /*[1], device*/, float* logp_out /*[B] or NULL*/, float* grad_out /*[B,N,3] or NULL*/,
                             float* report_out /*[B,GENIE_SYMMETRY_REPORT] or NULL*/, void* work, size_t work_bytes);
size_t genie_symmetry_potential_work_bytes(int B, int N);

/* The binder potential of twisted-diffusion / SMC sampling with its gradient and a per-particle report, without a handle: how a
 * design sits against a structure that is not being sampled (csrc/binder_kernels.hip) -- a receptor to bind, a hotspot patch to
 * cover, a partner to stay clear of.  Every other built-in potential looks at the design alone, and the denoiser has no input for an
 * external chain, so guidance is the only way to ask for this.  The reference has no counterpart.
 * The target is y_m, m = 0..M-1: C-alpha coordinates in Angstrom, fixed, in the frame the sampler works in (device memory, [M,3]).
 * hotspot is a list of H distinct target indices, ascending (device int32; H may be 0).  For particle b with coordinates x_n,
 * n = 0..N-1 (all N rows are used):
 *   d_nm = |x_n - y_m|
 *   s(d) = 1 / (1 + (d / contact_distance)^6)        (a rational switch, computed from d^2: no square root, no exp)
 *   E_clash   = clash_weight    * sum_{n,m} max(0, clash_distance - d_nm)^2
 *   C         = sum_{n,m} s(d_nm)
 *   E_contact = contacts_weight * ( max(0, contacts_min - C)^2 + max(0, C - contacts_max)^2 )     (contacts_max may be +inf)
 *   c_h       = sum_n s(d_{n,hotspot[h]})
 *   E_hot     = hotspot_weight  * sum_h max(0, hotspot_contacts - c_h)^2
 *   logp_out[b] = -(E_clash + E_contact + E_hot) / (2 var)
 *   grad_out[b,n] = d logp[b] / d x_n, analytic: with r = d / contact_distance, ds/dx_n = -6 r^4 s^2 (x_n - y_m) / contact_distance^2
 *         (no singularity), and k = contacts_weight ((C - contacts_max)_+ - (contacts_min - C)_+),
 *         grad[b,n] = (1/var) [ clash_weight sum_m (clash_distance - d_nm)_+ (x_n - y_m) / d_nm
 *                               + 6 / contact_distance^2 ( k sum_m r^4 s^2 (x_n - y_m)
 *                                                          - hotspot_weight sum_h (hotspot_contacts - c_h)_+ r^4 s^2 (x_n - y_hotspot[h]) ) ]
 * The unit vector of a clash pair is 0 where d is exactly 0 in float32, so every output is finite for finite inputs (coordinates
 * whose differences square to a finite float).  A weight of 0 switches its term off, energy and force.  `var` is one float in device
 * memory; the likelihood is left unnormalised.  The caller validates the hotspot list; an index is clamped into 0..M-1 all the same,
 * since it indexes LDS.  report_out[b] holds GENIE_BINDER_REPORT floats:
 *   contacts (C), n_contacts (pairs with d < contact_distance), n_interface (design residues with some target residue closer than
 *   contact_distance), target_min_distance (the smallest d_nm), n_target_clash (pairs with d < clash_distance),
 *   n_hotspots_contacted (hotspots with some design residue closer than contact_distance), e_target_clash, e_contact, e_hotspot
 *   (the weighted E above, before the division by 2 var)
 * (counts are stored as floats: exact up to 2^24; the names differ from the shape report's, so that a merged report keeps both).
 * hotspot_out [B,H], optional, receives the c_h.  logp_out and grad_out are given together or both NULL; report_out and hotspot_out
 * may be given alone; at least one output is asked for.
 * Two launches on `stream`: grid (ceil(N / 64), B), 256 threads; every work-group stages the target in dynamic LDS (12 M + 11 264
 * bytes; above 64 KiB the kernel's limit is raised) and takes 64 design residues, one per lane; each wave walks a contiguous quarter
 * of the target in partial sums of 64, the four wave sums are added in wave order, the c_h are reduced over the tile's lanes by
 * butterfly, and each residue's unscaled clash and contact force, the tile's 8 partial values and its 2 H hotspot values go to `work`
 * (genie_binder_potential_work_bytes(B, N, H) = 4 B (6 N + (8 + 2 H) ceil(N / 64)) bytes, 4-byte aligned).  The same grid with 64
 * threads then adds the tiles in tile order, forms the three hinge coefficients -- C and the c_h are global to the particle -- and
 * writes logp, the report, hotspot_out and the gradient, each residue adding its at most 64 hotspot pairs.  With clash_weight and
 * contacts_weight 0 and no report asked for the pair walk is skipped.  No allocation, no synchronisation, no host read, no atomics, no
 * scatter: every output is written once in a fixed order, so two calls on the same inputs are bitwise equal.
 * Returns GENIE_E_ARG, before the device is touched, with genie_last_error(NULL) naming this entry and the argument: B < 1 (or above
 * 65535); N < 1; M < 1; x0, target or var NULL; H outside 0..GENIE_BINDER_MAX_HOTSPOTS; H > 0 with a NULL hotspot; hotspot_out with
 * H = 0; a negative or non-finite distance, weight or count (contacts_max alone may be +inf); contacts_max below contacts_min; a
 * contact_distance of 0; no output asked for; logp_out and grad_out not given together; `work` NULL, misaligned or work_bytes too
 * small; an M whose staging does not fit in LDS (160 KiB: M above 12 714). */
#define GENIE_BINDER_REPORT 9   /* contacts, n_contacts, n_interface, target_min_distance, n_target_clash, n_hotspots_contacted,
                                   e_target_clash, e_contact, e_hotspot */
#define GENIE_BINDER_MAX_HOTSPOTS 64
int genie_binder_potential(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/, int M, const float* target /*[M,3], device*/,
                           int H, const int32_t* hotspot /*[H] device, ascending; NULL with H = 0*/,
                           float clash_distance, float clash_weight, float contact_distance, float contacts_min, float contacts_max,
                           float contacts_weight, float hotspot_contacts, float hotspot_weight, const float* var /*[1], device*/,
                           float* logp_out /*[B] or NULL*/, float* grad_out /*[B,N,3] or NULL*/,
                           float* report_out /*[B,GENIE_BINDER_REPORT] or NULL*/, float* hotspot_out /*[B,H] or NULL*/,
                           void* work, size_t work_bytes);
size_t genie_binder_potential_work_bytes(int B, int N, int H);

/* The TM-score of every pair of a set of M designs, without a handle (csrc/similarity_kernels.hip): what a diversity count of a
 * sampler's output is made of.  The score is the project's own and is stated here exactly; it is not a port of the TMscore or TMalign
 * programs and is a lower bound of theirs (gapless alignments only).  The reference has no counterpart.
 * x holds C-alpha coordinates in Angstrom, [M,N,3], design m using rows 0..length[m]-1 (the rest is never read); length is a device
 * int32 array with 4 <= length[m] <= N, validated by the caller (the kernel clamps it into 4..N all the same: it indexes memory).
 * One pair: the moving chain a has La residues, the fixed chain b has Lb, La <= Lb (equal lengths: the design with the lower index
 * moves).  At offset o in 0..Lb-La residue a_n corresponds to b_{o+n}.  Lnorm = La (norm 0, 'shorter') or Lb (norm 1, 'longer');
 *   d0(L) = max(0.5, 1.24 (L - 15)^(1/3) - 1.8) for L > 15, else 0.5;  d0 = d0(Lnorm).
 * Seeds: GENIE_TM_SEEDS = 11 windows over a's indices, in this order: (0, La); then for level k = 1, 2 the n_k = 2^(k+1) - 1 windows of
 * length len_k = max(ceil(La / 2^k), 4) that start at floor(j (La - len_k) / (n_k - 1)), j = 0..n_k-1.
 * Ascent from a seed, n_iter iterations: iteration 0 has weights w_n = 1 inside the window, 0 outside; every iteration takes the weighted
 * centroids c_p, c_q, the proper rotation R of Horn's quaternion of sum_n w_n (a_n - c_p)(b_{o+n} - c_q)^T (a mirror image does not fit),
 *   d_n^2 = |R (a_n - c_p) - (b_{o+n} - c_q)|^2 for all La residues,   score = (1 / Lnorm) sum_n 1 / (1 + d_n^2 / d0^2),
 * and hands w_n = (1 / (1 + d_n^2 / d0^2))^2 to the next one (the majorise-minimise step of the TM objective: in exact arithmetic the
 * score never decreases).  A seed's value is the largest score of its iterations, tm(a, b, o) the largest over the seeds, tm(a, b) the
 * largest over the offsets, ties to the lowest offset, then the lowest seed.
 *   tm[i,j] = tm[j,i] = tm(a, b);  offset[i,j] = offset[j,i] = the winning offset in the longer chain;
 *   rmsd[i,j] = rmsd[j,i] = sqrt(mean_n d_n^2) of seed 0, iteration 0 at the winning offset: the plain fit of all aligned residues.
 * The diagonal is written as tm 1, rmsd 0, offset 0 without being computed.
 * One launch on `stream`: grid (M, M), 256 threads, 28 N + 96 bytes of dynamic LDS; the work-groups below the diagonal return at once,
 * the one of pair i < j stages both chains in LDS, each centred on its own centroid, deals the (offset, seed) items to its four waves
 * in a fixed order, sums inside a wave by butterfly and writes both [i,j] and [j,i].  No allocation, no synchronisation, no host read,
 * no atomics, no work buffer: two calls on the same inputs are bitwise equal and the three matrices are exactly symmetric.
 * Returns GENIE_E_ARG, before anything is launched, with genie_last_error(NULL) naming this entry and the argument: M outside
 * 1..65535; N outside GENIE_TM_MIN_LENGTH..GENIE_TM_MAX_LENGTH; n_iter outside 1..GENIE_TM_MAX_ITER; a norm other than 0 or 1; a NULL
 * pointer. */
#define GENIE_TM_SEEDS 11
#define GENIE_TM_MIN_LENGTH 4
#define GENIE_TM_MAX_LENGTH 1706    /* the longest chain the samplers take */
#define GENIE_TM_MAX_ITER 32
int genie_pairwise_tm(genie_stream_t stream, int M, int N, const float* x /*[M,N,3]*/, const int* length /*[M], 4..N, device*/,
                      int norm /*0 shorter, 1 longer*/, int n_iter, float* tm /*[M,M]*/, float* rmsd /*[M,M]*/, int* offset /*[M,M]*/);

/* The fold potential of twisted-diffusion / SMC sampling with its gradient and a per-particle report, without a handle
 * (csrc/fold_kernels.hip): the score of genie_pairwise_tm between every particle and every one of R fixed reference backbones, kept
 * in a range per reference -- at or above a minimum for a template whose fold is wanted, at or below a maximum for folds to stay away
 * from.  It is the use of that score inside the sampling loop.  The reference has no counterpart.
 * Particles x0 [B,N,3], GENIE_TM_MIN_LENGTH <= N <= GENIE_TM_MAX_LENGTH; references ref [R,N,3], 1 <= R <= GENIE_FOLD_MAX_REFERENCES,
 * C-alpha coordinates in Angstrom of the same length N, fixed, in device memory; bounds [R,3] (device) holds per reference
 * (lo_r, hi_r, weight_r) with 0 <= lo_r <= hi_r, hi_r possibly +inf, weight_r >= 0, validated by the caller.
 * Score of a pair (b, r): the particle moves onto the reference under the identity alignment (gapless, offset 0); d0 = d0(N) and the
 * GENIE_TM_SEEDS windows over 0..N-1 are those of genie_pairwise_tm.  From seed s the ascent runs n_iter iterations exactly as stated
 * there: iteration 0 has weights 1 inside the window and 0 outside; every iteration takes the weighted centroids c_p, c_q, the proper
 * rotation R of Horn's quaternion of sum_n w_n (x_n - c_p)(y_n - c_q)^T,
 *   d_n^2 = |R (x_n - c_p) - (y_n - c_q)|^2 for all N residues,   g_n = 1 / (1 + d_n^2 / d0^2),
 * and hands w_n = g_n^2 to the next one.  The seed's value is sum_n g_n of its LAST iteration (genie_pairwise_tm takes the largest of
 * the iterations; the two are equal in exact arithmetic because the ascent is monotone, and the last is taken here so that the fit the
 * gradient uses is a fixed one, not whichever of several iterations equal to rounding happened to win).
 *   n_r = the largest value over the seeds, ties to the lowest seed;  (R*, c_p*, c_q*) = that seed's last fit;  tm_r = n_r / N
 *   E = sum_r weight_r [ max(0, N lo_r - n_r)^2 + max(0, n_r - N hi_r)^2 ]          (hinges on the soft number of superposed residues)
 *   logp_out[b] = -E / (2 var)
 *   grad_out[b,n] = d logp[b] / d x_n WITH EVERY PAIR'S WINNING RIGID TRANSFORM HELD FIXED:
 *         d n_r / d x_n = -(2 / d0^2) g_n^2 R*^T e_n,   e_n = R* (x_n - c_p*) - (y_n - c_q*),
 *         grad[b,n] = (2 / (var d0^2)) sum_r k_r g_n^2 R*^T e_n,   k_r = weight_r (max(0, n_r - N hi_r) - max(0, N lo_r - n_r)).
 * At a converged ascent the transform maximises the score, so this partial derivative is the total one (envelope theorem); nothing
 * differentiates through the iterations.  A reference whose hinges are both inactive, or whose weight is 0, contributes exactly 0 to
 * logp and to the gradient.  `var` is one float in device memory; the likelihood is left unnormalised.
 * report_out[b] holds GENIE_FOLD_REPORT floats: tm_nearest (max_r tm_r), nearest (the lowest r that attains it), tm_lowest_wanted
 * (min of tm_r over the references with lo_r > 0; 0 when there is none), n_fold_violations (references with max(0, N lo_r - n_r) or
 * max(0, n_r - N hi_r) positive, whatever their weight), e_fold (E, before the division by 2 var); counts are stored as floats.
 * tm_out [B,R], optional, receives tm_r.  logp_out and grad_out are given together or both NULL; report_out and tm_out may be given
 * alone; at least one output is asked for.
 * Two launches on `stream`.  Grid (R, B), 256 threads, 24 N + 344 bytes of dynamic LDS: the work-group of a pair stages both chains,
 * each centred on its own centroid, its four waves take the seeds w, w + 4, w + 8 with the lanes striding over the residues and
 * butterfly sums, and thread 0 writes n_r, the seed and the fit to `work` (genie_fold_potential_work_bytes(B, N, R) = 96 B R bytes,
 * 4-byte aligned) and tm_r to tm_out.  Grid (ceil(N / 256), B), 256 threads, launched when logp_out or report_out is given: one
 * thread per residue walks the references in index order and adds the energy, the report and, for references with k_r != 0 only,
 * its residue's share of the gradient under the stored fit.  No allocation, no synchronisation, no host read, no atomics, no scratch:
 * every output is written once in a fixed order, so two calls on the same inputs are bitwise equal.  Rows are never read out of range.
 * Returns GENIE_E_ARG, before anything is launched, with genie_last_error(NULL) naming this entry and the argument: B outside
 * 1..65535; N outside GENIE_TM_MIN_LENGTH..GENIE_TM_MAX_LENGTH; R outside 1..GENIE_FOLD_MAX_REFERENCES; n_iter outside
 * 1..GENIE_TM_MAX_ITER; x0, ref, bounds or var NULL; no output asked for; logp_out and grad_out not given together; `work` NULL,
 * misaligned or work_bytes too small. */
#define GENIE_FOLD_REPORT 5     /* tm_nearest, nearest, tm_lowest_wanted, n_fold_violations, e_fold */
#define GENIE_FOLD_MAX_REFERENCES 4096
int genie_fold_potential(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/, int R, const float* ref /*[R,N,3], device*/,
                         const float* bounds /*[R,3] device: lo, hi, weight*/, int n_iter, const float* var /*[1], device*/,
                         float* logp_out /*[B] or NULL*/, float* grad_out /*[B,N,3] or NULL*/,
                         float* report_out /*[B,GENIE_FOLD_REPORT] or NULL*/, float* tm_out /*[B,R] or NULL*/, void* work, size_t work_bytes);
size_t genie_fold_potential_work_bytes(int B, int N, int R);

/* Gapped TM alignment of M queries against R references, without a handle (csrc/tmalign_kernels.hip): the novelty of a design set (the
 * highest score of a design against known structures of any length) and a diversity count that an inserted loop does not throw.  The
 * score is the project's own and is stated here exactly; it is not a port of the TMalign program.  It is the TM-score of one explicit
 * alignment under one explicit superposition, so a lower bound of the true TM-score, and a tighter one than genie_pairwise_tm's.  The
 * reference has no counterpart.
 * xq [M,Nq,3] and xr [R,Nr,3] hold C-alpha coordinates in Angstrom; query m uses rows 0..lq[m]-1, reference r rows 0..lr[r]-1 (the rest
 * is never read); lq, lr are device int32 arrays with 4 <= length <= N, validated by the caller (the kernel clamps them into 4..N).
 * One pair: a = the shorter chain (equal lengths: the query), b = the longer chain, La <= Lb.  Lnorm = Lq, Lr, La, Lb for norm 0 (query),
 * 1 (reference), 2 (shorter), 3 (longer); d0 = d0(Lnorm) as for genie_pairwise_tm.
 * Stage 0, the seed, is genie_pairwise_tm's search of a along b: every offset o in 0..Lb-La, the GENIE_TM_SEEDS windows, n_iter
 * iterations of the weighted Horn ascent, the score (1 / Lnorm) sum_n 1 / (1 + d_n^2 / d0^2) over all La residues.  The winner is the
 * largest score over (offset, seed, iteration), ties to the lowest offset, then the lowest seed, then the earliest iteration; its
 * transform T (T x = R (x - c_p) + c_q) is kept and its alignment is the threading a_n <-> b_{o+n}.
 * Stages 1..n_rounds each start from the transform of the stage before:
 *   1. S_ij = 1 / (1 + |T a_i - b_j|^2 / d0^2) for i in 1..La, j in 1..Lb.
 *   2. The table: val(0, .) = val(., 0) = 0 and path(0, .) = path(., 0) = false (leading gaps are free);
 *        D = val(i-1, j-1) + S_ij,  H = val(i-1, j) + (path(i-1, j) ? gap_open : 0),  V = val(i, j-1) + (path(i, j-1) ? gap_open : 0);
 *      if D >= H and D >= V the move is diag, path = true, val = D; otherwise path = false, val = max(H, V) and the move is left (j-1)
 *      if V >= H, else up (i-1).
 *   3. Trace back from (La, Lb) along the moves until i = 0 or j = 0; every diag step aligns a_i with b_j.
 *   4. An alignment equal to the previous stage's (stage 0's threading included) stops the run: the stage is counted in `rounds`, not
 *      fitted.   5. Fewer than 3 aligned pairs stop it too.
 *   6. Otherwise n_iter iterations of the same ascent over the aligned pairs only: iteration 0 has weights 1, the score is
 *      (1 / Lnorm) sum_aligned 1 / (1 + d^2 / d0^2), the weights handed on are (1 / (1 + d^2 / d0^2))^2; the stage's value and transform
 *      are those of its best iteration, ties to the earliest.
 * The result is the stage with the largest value, ties to the earliest: tm[m,r] its value, rmsd[m,r] = sqrt(mean d^2) over its aligned
 * pairs under its transform, n_aligned[m,r] their number, rounds[m,r] the number of table fills run (n_rounds = 0: stage 0 alone, which
 * is genie_pairwise_tm's score with its alignment and transform).  map [M,R,Nq], optional: per query residue the matched reference
 * residue or -1 (-1 from lq[m] on).  rot [M,R,9] (row-major 3x3) and trans [M,R,3], optional and given together:
 * rot x_query + trans ~ x_reference, inverted when the reference was the moving chain.
 * One launch on `stream`: grid (R, M), 256 threads, one work-group per pair, at most 60 KB of dynamic LDS (both chains, T a, three
 * rolling diagonals of the table, three alignments and the moves of the whole table at 2 bits a cell).  The table is filled as an
 * anti-diagonal wavefront with S_ij formed on the fly; a row of the table has one owner thread, which stores its moves a whole dword
 * at a time.  No allocation, no synchronisation, no host read, no atomics, no work buffer, fixed summation trees: two calls on the same
 * inputs are bitwise equal.
 * Returns GENIE_E_ARG, before anything is launched, with genie_last_error(NULL) naming this entry and the argument: M or R outside
 * 1..65535; Nq or Nr outside GENIE_TM_MIN_LENGTH..GENIE_TMALIGN_MAX_LENGTH; Nq * Nr above GENIE_TMALIGN_MAX_CELLS; norm outside 0..3;
 * n_iter outside 1..GENIE_TM_MAX_ITER; n_rounds outside 0..GENIE_TMALIGN_MAX_ROUNDS; gap_open not finite, above 0 or below -10; a NULL
 * required pointer; rot without trans or trans without rot. */
#define GENIE_TMALIGN_MAX_LENGTH 1024
#define GENIE_TMALIGN_MAX_CELLS  131072     /* Nq * Nr of one call */
#define GENIE_TMALIGN_MAX_ROUNDS 16
int genie_tm_align(genie_stream_t stream, int M, int Nq, const float* xq /*[M,Nq,3]*/, const int* lq /*[M] device*/,
                   int R, int Nr, const float* xr /*[R,Nr,3]*/, const int* lr /*[R] device*/,
                   int norm, int n_iter, int n_rounds, float gap_open,
                   float* tm, float* rmsd, int* n_aligned, int* rounds /*each [M,R]*/,
                   int* map /*[M,R,Nq] or NULL*/, float* rot /*[M,R,9] or NULL*/, float* trans /*[M,R,3] or NULL*/);

/* The fold potential of twisted-diffusion / SMC sampling under gapped alignment, with its gradient and a per-particle report, without
 * a handle (csrc/fold_align_kernels.hip): genie_fold_potential with the identity alignment replaced by the alignment genie_tm_align
 * finds, so that a reference of any length counts and the score guidance pushes on is the score novelty reports.  The reference has
 * no counterpart.
 * Particles x0 [B,N,3]; references ref [R,Nr,3], reference r using rows 0..lr[r]-1 (the rest is never read), lr a device int32 array
 * with 4 <= lr[r] <= Nr, validated by the caller (the kernel clamps it into 4..Nr); bounds [R,3] (device) holds (lo_r, hi_r, weight_r)
 * as for genie_fold_potential.  norm (0 query, 1 reference, 2 shorter, 3 longer), n_iter, n_rounds and gap_open are genie_tm_align's;
 * offset_stride s >= 1.  For a pair (b, r), the particle being the query of length N and the reference of length L_r:
 *   1. Search.  genie_tm_align's procedure for (query x_b, reference y_r) exactly: stage 0, then stages 1..n_rounds, the best stage with
 *      ties to the earliest -- with one addition: stage 0 visits the offsets 0, s, 2 s, ... and always also the last one, Lb - La, in
 *      ascending order, ties to the lowest offset as before; at s = 1 the search IS genie_tm_align's.  Its results: the alignment A*
 *      (the map), the transform T* (rot0, trans0), n_aligned.
 *   2. Polish.  n_iter more iterations of the same weighted Horn ascent over the pairs of A* only, starting from the weights
 *      w = g(T*)^2 with g = 1 / (1 + d^2 / d0^2) under T*: every iteration takes the weighted centroids and the proper rotation of its
 *      weights, forms g under that fit and hands g^2 on.  The LAST iteration is taken, for genie_fold_potential's reason: the fit the
 *      gradient uses is a fixed one.  n_r = sum over the aligned pairs of g is the soft number of superposed residues, tm_r = n_r /
 *      Lnorm_r, and (R*, t*) is that fit written as R* x_query + t* ~ x_reference whichever chain moved.  In exact arithmetic the
 *      ascent is monotone, so n_r / Lnorm_r >= genie_tm_align's tm.
 *   3. Energy.  E = sum_r weight_r [ max(0, Lnorm_r lo_r - n_r)^2 + max(0, n_r - Lnorm_r hi_r)^2 ],  logp_out[b] = -E / (2 var), var
 *      one float in device memory.
 *   4. Gradient, WITH EVERY PAIR'S ALIGNMENT A* AND FIT (R*, t*) HELD FIXED.  For a query residue i aligned to reference residue j:
 *         e_i = R* x_i + t* - y_j,   d n_r / d x_i = -(2 / d0_r^2) g_i^2 R*^T e_i;   an unaligned residue gets 0;
 *         grad_out[b,i] = (2 / var) sum_r (k_r / d0_r^2) g_i^2 R*^T e_i,   k_r = weight_r (max(0, n_r - Lnorm_r hi_r) - max(0, Lnorm_r lo_r - n_r)),
 *      d0_r = d0(Lnorm_r), which differs between references unless norm is 0 (query).
 *      The alignment is piecewise constant in x, so this is the derivative on the piece the particle lies in: where the alignment
 *      changes the score has a kink and the gradient says nothing about the other side.  The envelope theorem covers the fit (at a
 *      converged ascent it maximises n_r over rigid transforms, so holding it fixed gives the total derivative on the piece).  Nothing
 *      differentiates through the table, the traceback or the iterations.  A reference whose hinges are both inactive, or whose weight
 *      is 0, contributes exactly 0 to logp and to the gradient.
 *   5. Report.  report_out[b] holds GENIE_FOLD_REPORT floats with genie_fold_potential's meaning, `N lo` there reading `Lnorm_r lo`
 *      here: tm_nearest, nearest, tm_lowest_wanted, n_fold_violations, e_fold.
 * Optional outputs, each may be NULL: tm_out [B,R] (tm_r); n_aligned_out [B,R] int32; map_out [B,R,N] int32, per query residue the
 * matched reference residue or -1; rot_out [B,R,9] (row-major) and trans_out [B,R,3], given together: the polished fit (R*, t*);
 * rot0_out and trans0_out, given together: T* before the polish.  logp_out and grad_out are given together or both NULL; at least one
 * output is asked for.
 * Two launches on `stream`.  Grid (R, B), 256 threads, one work-group per pair, genie_tm_align's LDS layout (at most 60 KB of dynamic
 * LDS) and anti-diagonal wavefront; wave 0 runs the polish; the pair's n_r, Lnorm_r, d0_r and fit (20 floats) and its query-indexed map
 * (N int32, inverted through LDS when the reference moved) go to `work`: genie_fold_align_potential_work_bytes(B, N, R) =
 * 4 B R (20 + N) bytes, 4-byte aligned (0 for B, N or R out of range).  Grid (ceil(N / 256), B), 256 threads, launched when logp_out
 * or report_out is given: one thread per query residue walks the references in index order, reads its map entry and the stored fit and
 * adds the energy, the report and, for references with k_r != 0 only, its residue's share of the gradient.  No allocation, no
 * synchronisation, no host read, no atomics, no scratch, fixed summation order: two calls on the same inputs are bitwise equal.  Rows
 * are never read out of range.
 * Returns GENIE_E_ARG, before anything is launched, with genie_last_error(NULL) naming this entry and the argument: B outside
 * 1..65535; N or Nr outside GENIE_TM_MIN_LENGTH..GENIE_TMALIGN_MAX_LENGTH; N * Nr above GENIE_TMALIGN_MAX_CELLS; R outside
 * 1..GENIE_FOLD_ALIGN_MAX_REFERENCES; norm outside 0..3; n_iter outside 1..GENIE_TM_MAX_ITER; n_rounds outside
 * 0..GENIE_TMALIGN_MAX_ROUNDS; gap_open not finite, above 0 or below -10; offset_stride outside 1..GENIE_FOLD_ALIGN_MAX_STRIDE; x0,
 * ref, lr, bounds or var NULL; no output asked for; logp_out without grad_out, rot_out without trans_out, rot0_out without trans0_out
 * or the other way round; `work` NULL, misaligned or work_bytes too small. */
#define GENIE_FOLD_ALIGN_MAX_REFERENCES 1024
#define GENIE_FOLD_ALIGN_MAX_STRIDE 64
int genie_fold_align_potential(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/,
                               int R, int Nr, const float* ref /*[R,Nr,3], device*/, const int* lr /*[R] device*/,
                               const float* bounds /*[R,3] device: lo, hi, weight*/,
                               int norm, int n_iter, int n_rounds, float gap_open, int offset_stride, const float* var /*[1], device*/,
                               float* logp_out /*[B] or NULL*/, float* grad_out /*[B,N,3] or NULL*/,
                               float* report_out /*[B,GENIE_FOLD_REPORT] or NULL*/, float* tm_out /*[B,R] or NULL*/,
                               int* n_aligned_out /*[B,R] or NULL*/, int* map_out /*[B,R,N] or NULL*/,
                               float* rot_out /*[B,R,9] or NULL*/, float* trans_out /*[B,R,3] or NULL*/,
                               float* rot0_out /*[B,R,9] or NULL*/, float* trans0_out /*[B,R,3] or NULL*/, void* work, size_t work_bytes);
size_t genie_fold_align_potential_work_bytes(int B, int N, int R);

/* The diversity potential of twisted-diffusion / SMC sampling with its gradient and a per-particle report, without a handle
 * (csrc/diversity_kernels.hip): the particles of one batch repel each other, so that the designs of one run do not come out as
 * near-copies.  It is genie_fold_potential with the batch itself for the references.  The reference has no counterpart.
 * The batch is x0 [B,N,3], 1 <= B <= GENIE_DIVERSITY_MAX_BATCH, GENIE_TM_MIN_LENGTH <= N <= GENIE_TM_MAX_LENGTH, laid out system-major:
 * K in 1..64 divides B, S = B / K, sys(b) = b / K (genie_smc_reweight's layout).  The constants are tm_max in (0, 1], weight > 0,
 * n_iter and var (one float in device memory).  d0 = d0(N); the GENIE_TM_SEEDS seed windows are those of genie_pairwise_tm.
 * Pairs.  For every i < j with sys(i) != sys(j), genie_fold_potential's procedure exactly, x_i the particle (it moves) and x_j the
 * reference: GENIE_TM_SEEDS seeds, n_iter iterations each, the value sum_n g_n of the LAST iteration, the best seed (ties to the
 * lowest) giving n_ij and the fit (R, c_p, c_q).  n_ji := n_ij: every unordered pair is scored once, and its one fit serves both
 * members (in float64 the score with j moving instead is the same to 1e-14 N on the test inputs).  Particles of one system are
 * resampled copies of each other and are not scored.  tm_out [B,B], optional, receives n_ij / N at [i,j] and at [j,i] and 0 at the
 * same-system entries, the diagonal included; all of it is written on every call.
 * Energy.  a_bj = max(0, n_bj - N tm_max);  E_b = (weight / K) sum_{j: sys(j) != sys(b)} a_bj^2;  logp_out[b] = -E_b / (2 var).
 * Gradient.  grad_out[b,n] = d logp_b / d x_{b,n} WITH EVERY OTHER PARTICLE AND EVERY FIT HELD FIXED: the particle's own twisting
 * function, the others being parameters.  With c = 2 weight / (K var d0^2) and g_n = 1 / (1 + |e_n|^2 / d0^2):
 *   j > b (b moved in the pair's fit):          e_n = R (x_{b,n} - c_p) - (x_{j,n} - c_q),   + c a_bj g_n^2 R^T e_n
 *   j < b (b was the reference of pair (j, b)): e_n = R (x_{j,n} - c_p) - (x_{b,n} - c_q),   - c a_bj g_n^2 e_n
 * A pair with a_bj = 0 contributes exactly 0.  With S = 1, logp and grad are exactly 0 and nothing is fitted.
 * report_out[b] holds GENIE_DIVERSITY_REPORT floats: tm_nearest_design (the largest n_bj / N over the scored partners; 0 when there
 * is none), nearest_design (the lowest j that attains it; -1 when there is none), tm_mean_design (the mean over the scored partners;
 * 0 when there is none), n_similar (partners with a_bj > 0), e_diversity (E_b, before the division by 2 var); counts are stored as
 * floats.  logp_out and grad_out are given together or both NULL; report_out and tm_out may be given alone; at least one output is
 * asked for.
 * Two launches on `stream`.  One 256-thread work-group per unordered pair (pair (i, j), i < j, is work-group and slot
 * j (j - 1) / 2 + i; a pair inside one system returns at once), 24 N + 344 bytes of dynamic LDS, the arithmetic of
 * genie_fold_potential's fit kernel operation for operation: thread 0 writes n, the seed, the fit and the two staged centroids, 24
 * floats, to the pair's slot of `work` (genie_diversity_potential_work_bytes(B, K, N) = 96 max(1, B (B - 1) / 2) bytes, 4-byte
 * aligned; 0 for sizes this entry refuses) and both tm_out entries; it is skipped when S = 1.  Grid (ceil(N / 256), B), 256 threads,
 * one thread per residue: it walks the partners j in index order, looks the pair's fit up and adds the energy, the report and, for
 * pairs with a_bj > 0 only, the moving-side or reference-side term; thread 0 of tile 0 writes logp, the report and tm_out's zeros.
 * No allocation, no synchronisation, no host read, no atomics, no scratch: every output is written once in a fixed order, so two calls
 * on the same inputs are bitwise equal.  Rows n >= N and the same-system slots of `work` are never read.
 * Returns GENIE_E_ARG, before anything is launched, with genie_last_error(NULL) naming this entry and the argument: B outside
 * 1..GENIE_DIVERSITY_MAX_BATCH (so that B (B - 1) / 2 <= 2^20 pairs and 96 MB of work); K outside 1..64 or not dividing B; N outside
 * GENIE_TM_MIN_LENGTH..GENIE_TM_MAX_LENGTH; n_iter outside 1..GENIE_TM_MAX_ITER; tm_max not in (0, 1]; weight not finite or negative;
 * x0 or var NULL; no output asked for; logp_out and grad_out not given together; `work` NULL, misaligned or work_bytes too small. */
#define GENIE_DIVERSITY_REPORT 5     /* tm_nearest_design, nearest_design, tm_mean_design, n_similar, e_diversity */
#define GENIE_DIVERSITY_MAX_BATCH 1448
int genie_diversity_potential(genie_stream_t stream, int B, int K, int N, const float* x0 /*[B,N,3]*/, float tm_max, float weight,
                              int n_iter, const float* var /*[1], device*/, float* logp_out /*[B] or NULL*/,
                              float* grad_out /*[B,N,3] or NULL*/, float* report_out /*[B,GENIE_DIVERSITY_REPORT] or NULL*/,
                              float* tm_out /*[B,B] or NULL*/, void* work, size_t work_bytes);
size_t genie_diversity_potential_work_bytes(int B, int K, int N);

/* The burial potential of twisted-diffusion / SMC sampling with its gradient and a per-particle report, without a handle
 * (csrc/burial_kernels.hip): which residues lie inside the design and which on its surface.  On a C-alpha model that is the
 * half-sphere exposure (HSE-alpha): the number of C-alpha atoms in the half sphere that the virtual C-beta direction points into.
 * Every other built-in potential is blind to inside and outside.  The reference has no counterpart.
 * For particle b with C-alpha coordinates x_n, n = 0..N-1 (all N rows are used):
 *   b_n   = 2 x_n - x_{n-1} - x_{n+1}  for 1 <= n <= N-2;  b_0 = b_{N-1} = 0          (the ends have no direction)
 *   rho_n = sqrt(|b_n|^2 + eps^2),  u_n = b_n / rho_n          (eps = GENIE_BURIAL_EPS, 0.1 A: smooth where the chain is straight)
 *   for every ordered pair n, j with |j - n| >= separation:
 *     r = x_j - x_n,  q = |r|^2
 *     s = 1 / (1 + (q / radius^2)^3)                 (genie_binder_potential's rational switch: from q, no square root, no exp)
 *     h = u_n . r
 *     g = 1/2 (1 + h / sqrt(h^2 + width^2))          (a soft half-space: 1/2 on the plane through x_n, -> 1 on the side-chain side)
 *   c_n   = sum_j s g                                (the soft half-sphere count of residue n; ends: half the soft full-sphere count)
 *   m     = (1/N) sum_n c_n
 *   E_res  = sum_n w_n [ (lo_n - c_n)_+^2 + (c_n - hi_n)_+^2 ]        (per-residue table lo, hi, w [N]; hi may be +inf, w_n = 0: no target)
 *   E_mean = mean_weight [ (mean_min - m)_+^2 + (m - mean_max)_+^2 ]  (mean_max may be +inf)
 *   logp_out[b] = -(E_res + E_mean) / (2 var)
 * grad_out[b,i] = d logp[b] / d x_i, analytic.  With k_n = w_n [(c_n - hi_n)_+ - (lo_n - c_n)_+] + (mean_weight / N) [(m - mean_max)_+
 * - (mean_min - m)_+]:
 *   f_nj = g ds/dr + s g' u_n,   ds/dr = -6 (q / radius^2)^2 s^2 r / radius^2,   g' = 1/2 width^2 / (h^2 + width^2)^(3/2)
 *   a_n  = sum_j s g' r                                   (the pull on the direction u_n)
 *   v_n  = (a_n - u_n (u_n . a_n)) / rho_n                (0 at the two ends)
 *   grad[b,i] = -(1/var) [ sum_n k_n f_ni - k_i sum_j f_ij + 2 k_i v_i - k_{i-1} v_{i-1} - k_{i+1} v_{i+1} ]
 * with k and v outside 0..N-1 taken as 0.  Nothing is divided by a distance: coincident residues, a straight chain (b_n = 0) and all
 * residues in one point give finite outputs; the force of a pair with q / radius^2 >= 1e12 is taken as 0 (it is below 1e-48).  lo, hi
 * and w are device arrays of N floats, given together or all NULL (no per-residue term); the caller validates them (0 <= lo <= hi,
 * w >= 0 and finite).  `var` is one float in device memory; the likelihood is left unnormalised.  report_out[b] holds
 * GENIE_BURIAL_REPORT floats:
 *   burial_mean (m), burial_min, burial_max (the smallest and the largest c_n), n_burial_violated (residues with w_n > 0 and c_n
 *   outside lo_n..hi_n), max_burial_violation (the largest (lo_n - c_n)_+ or (c_n - hi_n)_+ over the residues with w_n > 0),
 *   e_burial_target (E_res), e_burial_mean (E_mean) (weighted, before the division by 2 var)
 * (the count is stored as a float; the names differ from every other report's, so that a merged report keeps them all).  burial_out
 * [B,N], optional, receives the c_n.  logp_out and grad_out are given together or both NULL; report_out and burial_out may be given
 * alone; at least one output is asked for.
 * Three launches on `stream`, the second only with grad_out.  Counts: grid (ceil(N / 64), B), 256 threads; every work-group stages
 * the particle's x and u in dynamic LDS (24 N + 1024 bytes) and takes 64 centres n, one per lane; each wave walks a contiguous
 * quarter of the neighbours j (wave-uniform: an LDS broadcast) in partial sums of 64, the four wave sums are added in wave order, and
 * c_n goes to `work`.  Forces: the same grid; x, u, rho and k of the whole particle are staged (32 N + 10 240 bytes; every
 * work-group forms m from the c_n in one fixed order), lane i walks the pairs again, once as the centre (a_i and sum_j f_ij) and once
 * as the neighbour of centre j (k_j f_ji, skipped where k_j = 0), and stores sum_n k_n f_ni - k_i sum_j f_ij and k_i v_i, 6 floats.
 * Stencil: grid (ceil(N / 256), B), 256 threads, one residue per thread: the three-residue sum above; work-group 0 of the particle
 * reduces the c_n in a fixed order and writes logp and the report.  `work` holds 7 N floats per particle
 * (genie_burial_potential_work_bytes(B, N) = 28 B N bytes, 4-byte aligned; 0 for sizes this entry refuses).  No allocation, no
 * synchronisation, no host read, no atomics, no scatter: every output is written once in a fixed order, so two calls on the same
 * inputs are bitwise equal.
 * Returns GENIE_E_ARG, before the device is touched, with genie_last_error(NULL) naming this entry and the argument: B < 1 (or above
 * 65535); N < 1 or above GENIE_BURIAL_MAX_LENGTH (1728: the forces' staging fills the 64 KiB of LDS a kernel gets without asking); x0
 * or var NULL; separation < 1; radius or width not finite or <= 0 (or radius^2 no normal float); one or two of lo, hi, w given; a
 * negative or non-finite mean_weight, mean_min or mean_max (mean_max alone may be +inf); mean_max below mean_min; logp_out asked for
 * with no term enabled (no table and mean_weight 0); no output asked for; logp_out and grad_out not given together; `work` NULL,
 * misaligned or work_bytes too small. */
#define GENIE_BURIAL_REPORT 7   /* burial_mean, burial_min, burial_max, n_burial_violated, max_burial_violation, e_burial_target,
                                   e_burial_mean */
#define GENIE_BURIAL_EPS 0.1f
#define GENIE_BURIAL_MAX_LENGTH 1728
int genie_burial_potential(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/, float radius, float width, int separation,
                           const float* lo, const float* hi, const float* w /*[N] each, device; all three NULL: no per-residue term*/,
                           float mean_min, float mean_max, float mean_weight, const float* var /*[1], device*/,
                           float* logp_out /*[B] or NULL*/, float* grad_out /*[B,N,3] or NULL*/,
                           float* report_out /*[B,GENIE_BURIAL_REPORT] or NULL*/, float* burial_out /*[B,N] or NULL: the c_n*/,
                           void* work, size_t work_bytes);
size_t genie_burial_potential_work_bytes(int B, int N);

/* The envelope potential of twisted-diffusion / SMC sampling with its gradient and a per-particle report, without a handle
 * (csrc/envelope_kernels.hip): what shape the design should have.  An envelope is M points y_m (device, [M,3]) with weights v_m > 0
 * (device, [M]; NULL: all 1), in the frame the sampler works in: the lattice points of a solid, the atoms of an existing protein, the
 * pseudo-atoms of a low-resolution map.  The design is kept inside it and made to fill it, by a soft assignment in both directions.
 * The reference has no counterpart.
 * For particle b with C-alpha coordinates x_n, n = 0..N-1, tau = softness (A^2), eps = GENIE_ENVELOPE_EPS (0.1 A) and
 * q_nm = |x_n - y_m|^2, always formed from the coordinate differences, never from expanded norms:
 *   s_n = -tau log sum_m exp(-q_nm / tau)       (the soft minimum over the points)     a_n = sqrt(max(s_n, 0) + eps^2)
 *   t_m = -tau log sum_n exp(-q_nm / tau)       (the soft minimum over the residues)   c_m = sqrt(max(t_m, 0) + eps^2)
 *   stay inside:  h_n = max(0, a_n - inside_distance),   E_inside = inside_weight sum_n h_n^2
 *   fill it:      g_m = max(0, c_m - cover_distance),    E_cover  = cover_weight (N / sum v) sum_m v_m g_m^2
 *   logp_out[b] = -(E_inside + E_cover) / (2 var)
 * With p_nm = exp((s_n - q_nm) / tau) and r_nm = exp((t_m - q_nm) / tau), both <= 1:
 *   grad_out[b,n] = -(1/var) [ inside_weight (h_n / a_n) sum_m p_nm (x_n - y_m) + cover_weight (N / sum v) sum_m v_m (g_m / c_m) r_nm (x_n - y_m) ]
 * Both distances exceed eps, so the clamp at s = 0 (t = 0) lies where the hinge is 0 and E is C^1.  Both log-sum-exps subtract the
 * running minimum: no exponential is taken of a positive number, and a particle hundreds of Angstrom from the envelope -- where a
 * design is at high noise -- underflows nothing.  A weight of 0 switches its term off: its energy is exactly 0 and its exponentials
 * in the gradient are not taken.  `var` is one float in device memory; the likelihood is left unnormalised.  eps is the compile-time
 * constant, not an argument.  report_out[b] holds GENIE_ENVELOPE_REPORT floats:
 *   n_outside (residues with h_n > 0), max_outside (the largest h_n), n_uncovered (points with g_m > 0), max_uncovered (the largest
 *   g_m), e_envelope_inside (E_inside), e_envelope_cover (E_cover) (weighted, before the division by 2 var; counts stored as floats).
 * distance_out [B,N], optional, receives the a_n; gap_out [B,M], optional, the c_m.  logp_out and grad_out are given together or both
 * NULL; the others may be given alone; at least one output is asked for.
 * Three launches on `stream`, the second only with grad_out, the third only with logp_out or report_out.  Soft minima: grid
 * (ceil(N / 64) + ceil(M / 64), B), W waves: one loop with the roles swapped -- a work-group owns 64 residues, one per lane, and
 * walks the points, or owns 64 points and walks the particle's residues.  The walked side is staged through 16 KiB of LDS in chunks
 * of GENIE_ENVELOPE_CHUNK rows; each of the W waves takes a contiguous W-th of a chunk (wave-uniform row: an LDS broadcast),
 * first for its smallest q, then for the sum of exp((min - q) / tau); a lane carries a (running minimum, rescaled sum) pair and the waves'
 * pairs are merged in wave order.  s_n, t_m, the coefficients cover_weight (N / sum v) v_m g_m / c_m and three sums per tile go to
 * `work`.  Gather: grid (ceil(N / 64), B): lane n walks the points again, staged with t_m and the coefficient, and skips the
 * exponential of p_nm where h_n = 0 and that of r_nm where the point's coefficient is 0.  Finish: grid (B): the tile sums are added
 * in tile order; logp and the report.  W = 16, so that the few work-groups of a small batch finish their serial walks sooner (B = 8,
 * N = 256, M = 2048: 288 work-groups on 256 compute units); a launch of GENIE_ENVELOPE_FILL work-groups or more fills the device
 * without that and uses W = 4.  The choice depends on B, N and M alone, so equal calls stay bitwise equal; a particle's last bits
 * may differ between batch sizes on either side of the threshold.  B N M exponentials for each soft minimum and at most 2 B N M for the gather.  `work` holds
 * N + 2 M + 3 (ceil(N / 64) + ceil(M / 64)) floats per particle (genie_envelope_potential_work_bytes(B, N, M), 4-byte aligned; 0 for
 * sizes this entry refuses).  No allocation, no synchronisation, no host read, no atomics, no scatter: every output is written once
 * in a fixed order, so two calls on the same inputs are bitwise equal.
 * Limits.  No LDS or register limit bounds N or M, since the walked side is staged in chunks.  B <= 65535 is the grid's y extent.
 * N <= GENIE_ENVELOPE_MAX_LENGTH (4096) and M <= GENIE_ENVELOPE_MAX_POINTS (16384) bound the time of a call -- at both limits one
 * particle takes 2^28 exponentials on the quarter-rate transcendental pipe -- and the finishing step's tile table (320 tiles, 3840
 * bytes of LDS).
 * Returns GENIE_E_ARG, before the device is touched, with genie_last_error(NULL) naming this entry and the argument: B outside
 * 1..65535; N outside 1..GENIE_ENVELOPE_MAX_LENGTH; M outside 1..GENIE_ENVELOPE_MAX_POINTS; x0, points or var NULL; softness not
 * finite or <= 0; inside_distance or cover_distance not finite or <= eps; a negative or non-finite weight; both weights 0; no output
 * asked for; logp_out and grad_out not given together; `work` NULL, misaligned or work_bytes too small.  The caller validates the
 * point weights (finite, > 0). */
#define GENIE_ENVELOPE_REPORT 6   /* n_outside, max_outside, n_uncovered, max_uncovered, e_envelope_inside, e_envelope_cover */
#define GENIE_ENVELOPE_EPS 0.1f
#define GENIE_ENVELOPE_CHUNK 1024
#define GENIE_ENVELOPE_FILL 2048  /* work-groups of a launch from which it runs 4 waves per work-group instead of 16 */
#define GENIE_ENVELOPE_MAX_LENGTH 4096
#define GENIE_ENVELOPE_MAX_POINTS 16384
int genie_envelope_potential(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/, int M, const float* points /*[M,3], device*/,
                             const float* weights /*[M], device, or NULL: all 1*/, float softness, float inside_distance,
                             float inside_weight, float cover_distance, float cover_weight, const float* var /*[1], device*/,
                             float* logp_out /*[B] or NULL*/, float* grad_out /*[B,N,3] or NULL*/,
                             float* report_out /*[B,GENIE_ENVELOPE_REPORT] or NULL*/, float* distance_out /*[B,N] or NULL: the a_n*/,
                             float* gap_out /*[B,M] or NULL: the c_m*/, void* work, size_t work_bytes);
size_t genie_envelope_potential_work_bytes(int B, int N, int M);

/* The context potential of twisted-diffusion / SMC sampling with its gradient, a per-particle report and the fitted pose, without a
 * handle (csrc/context_kernels.hip): a binding partner that follows each particle's own placement of the motif.  The motif's anchors
 * are superposed on the design residues that hold them, the fitted rigid motion places the partner's C-alpha atoms (the context),
 * and the placed context is scored against the rest of the design with genie_binder_potential's clash and contact terms.  The
 * reference has no counterpart.
 * anchor_index [B,A] (device int32) names, per particle, the A distinct design residues idx[k] that hold the anchors; anchor_xyz
 * [A,3] are the anchors' coordinates t_k and context [C,3] the context's y_c, both in one frame (the motif file's; device memory).
 * For particle b with coordinates x_n, n = 0..N-1:
 *   a_k = x_idx[k],  abar = mean_k a_k,  tbar = mean_k t_k
 *   S   = sum_k (t_k - tbar)(a_k - abar)^T                         (S_ab = sum t_a c_b)
 *   q   = the unit eigenvector of the largest eigenvalue lam_0 of Horn's symmetric 4x4 K(S), float32 Jacobi (csrc/horn.h: mr_eigen),
 *   R   = R(q), the proper rotation that minimises sum_k |R (t_k - tbar) - (a_k - abar)|^2
 *   y'_c = R (y_c - tbar) + abar                                   (the context as placed for this particle)
 *   anchor_rmsd = sqrt(mean_k |R (t_k - tbar) - (a_k - abar)|^2)
 *   over the pairs (n, c) with n NOT an anchor:  d = |x_n - y'_c|,  s(d) = 1 / (1 + (d / contact_distance)^6)
 *   E_clash   = clash_weight    * sum max(0, clash_distance - d)^2
 *   Cc        = sum s(d)
 *   E_contact = contacts_weight * ( max(0, contacts_min - Cc)^2 + max(0, Cc - contacts_max)^2 )    (contacts_max may be +inf)
 *   logp_out[b] = -(E_clash + E_contact) / (2 var)
 * Anchors are left out of the pair sums: the geometry between motif and partner is given.  grad_out[b,n] = d logp[b] / d x_n is the
 * exact gradient of this function with the anchor rows held fixed.  With p_nc the force of pair (n, c) on x_n,
 *   p_nc = clash_weight (clash_distance - d)_+ (x_n - y'_c) / d + 6 k / contact_distance^2 r^4 s^2 (x_n - y'_c),
 *   k = contacts_weight ((Cc - contacts_max)_+ - (contacts_min - Cc)_+),  r = d / contact_distance
 * (0 for a clash pair with d exactly 0), P = sum_nc p_nc and M = sum_nc p_nc (y'_c - abar)^T:
 *   grad[b,n]      = (1/var) sum_c p_nc                                        for n not an anchor
 *   grad[b,idx[k]] = (1/var) ( -P / A + D^T (t_k - tbar) )                     for the anchors
 * where D = dE/dS follows from G_R = -M R (the derivative with respect to R: the reaction -p_nc on y'_c times (y_c - tbar)^T) by
 * first-order perturbation of the top eigenvector (csrc/horn.h: mr_fit_adjoint): g = dR/dq : G_R without its component along q,
 * z = sum_{i=1..3} v_i (v_i . g) / (lam_0 - lam_i) over the three other eigenpairs, dE/dK_ij = z_i q_j, and K is linear in S.  An
 * eigenpair with lam_0 - lam_i not above 1e-6 lam_0 (MR_GAP_FLOOR) contributes 0: a degenerate fit (anchors on one line, or all
 * at one point) has no unique rotation, and every output stays finite.  Net force and net torque of the gradient are 0.
 * report_out[b] holds GENIE_CONTEXT_REPORT floats:
 *   context_contacts (Cc), n_context_contacts (pairs with d < contact_distance), n_context_interface (design residues, anchors
 *   excluded, with some context atom closer than contact_distance), context_min_distance (the smallest d; +inf when A = N leaves no
 *   pair), n_context_clash (pairs with d < clash_distance), anchor_rmsd, e_context_clash, e_context_contact (the weighted E above,
 *   before the division by 2 var)
 * (counts are stored as floats: exact up to 2^24; the names differ from the binder report's, so that a merged report keeps both).
 * pose_out[b], optional, receives R row-major and then the translation abar - R tbar: y' = R y + t.  logp_out and grad_out are given
 * together or both NULL; report_out and pose_out may be given alone (pose_out alone runs the fit only); at least one output is asked
 * for.  A weight of 0 switches its term off, energy and force.
 * The anchor rows are checked on the device: a row with an index outside 0..N-1 (clamped before it is used as an address) or with an
 * index given twice flags its particle, which gets logp 0, a gradient of 0, a report of 0 and the identity pose.
 * Three launches on `stream`.  The fit: grid B, one wave per particle, lanes striding over the anchors; it leaves R, abar, tbar, the
 * four eigenpairs, anchor_rmsd, the flag and a residue-to-anchor map in `work`.  The pairs: grid (ceil(N / 64), B), 256 threads;
 * every work-group stages R (y_c - tbar) in dynamic LDS (12 C + 11 552 bytes; above 64 KiB the kernel's limit is raised) and takes 64
 * design residues, one per lane; each wave walks a contiguous quarter of the context in partial sums of 64, every lane keeping the
 * 2 x 9 moments of p_nc beside the binder kernel's sums; each residue's unscaled clash and contact force and the tile's 30 partial
 * values go to `work` (genie_context_potential_work_bytes(B, N) = 4 B (40 + 7 N + 32 ceil(N / 64)) bytes, 4-byte aligned).  The
 * finish: the same grid with 64 threads adds the tiles in tile order, forms k, P, M and D, and writes logp, the report and the
 * gradient, an anchor its share instead of a direct force.  No allocation, no synchronisation, no host read, no atomics, no scatter:
 * every output is written once in a fixed order, so two calls on the same inputs are bitwise equal.
 * Returns GENIE_E_ARG, before the device is touched, with genie_last_error(NULL) naming this entry and the argument: B < 1 (or above
 * 65535); N < 1; A outside 3..N; C < 1; x0, anchor_index, anchor_xyz, context or var NULL; a negative or non-finite distance, weight
 * or count (contacts_max alone may be +inf); contacts_max below contacts_min; a contact_distance of 0; no output asked for; logp_out
 * and grad_out not given together; `work` NULL, misaligned or work_bytes too small; a C whose staging does not fit in LDS (160 KiB:
 * C above GENIE_CONTEXT_MAX_ATOMS). */
#define GENIE_CONTEXT_REPORT 8   /* context_contacts, n_context_contacts, n_context_interface, context_min_distance, n_context_clash,
                                    anchor_rmsd, e_context_clash, e_context_contact */
#define GENIE_CONTEXT_MAX_ATOMS 12690
int genie_context_potential(genie_stream_t stream, int B, int N, const float* x0 /*[B,N,3]*/, int A,
                            const int32_t* anchor_index /*[B,A], device*/, const float* anchor_xyz /*[A,3], device*/, int C,
                            const float* context /*[C,3], device*/, float clash_distance, float clash_weight, float contact_distance,
                            float contacts_min, float contacts_max, float contacts_weight, const float* var /*[1], device*/,
                            float* logp_out /*[B] or NULL*/, float* grad_out /*[B,N,3] or NULL*/,
                            float* report_out /*[B,GENIE_CONTEXT_REPORT] or NULL*/, float* pose_out /*[B,12] or NULL*/, void* work,
                            size_t work_bytes);
size_t genie_context_potential_work_bytes(int B, int N);

/* Denoiser.forward (genie/model/model.py:125-192): z_out[B,N,3].
 * timesteps: device int32 [B].  quat_codes: optional device int8 [B,N,N]
 * pinning the sign of each pair quaternion to the reference's eigh output
 * (SURVEY.md hazard 1): 0 = canonical, else 1 + 2*m + neg = "component m has
 * sign (neg ? - : +)".
 * With n_head_tri > 0 every pair transform layer also runs the two triangular attention modules
 * (csrc/pair_triatt_kernels.hip), in both arithmetic modes; so do genie_p_sample's and genie_sample_loop's calls. */
int genie_denoise(genie_handle_t h, genie_stream_t stream,
                  const float* trans, const float* rots, const int32_t* timesteps,
                  const int8_t* quat_codes, float* z_out, const genie_taps_t* taps);

/* One ancestral step of BaseSampler._sample (genie/sampler/base.py:249-282):
 * trans <- ((trans - w_z z)/sqrt(alpha_t) * mask [+ scale sqrt(beta_t) eps]) * mask,
 * then Frenet frames.  eps == NULL for step 1. */
int genie_p_sample(genie_handle_t h, genie_stream_t stream, int step, float scale,
                   float* trans_inout, float* rots_out, const float* z, const float* eps);

/* The whole reverse loop (genie/sampler/base.py:227-282), device resident.
 * noise [n_timestep][B,N,3]: noise[0] is the initial trans (base.py:227),
 * noise[k] the draw of iteration k (steps T..2).  first_step/last_step allow a
 * partial trajectory (T..1 for the full one); when first_step < T,
 * trans_io/rots_io carry the state in.  noise is indexed by the timestep and
 * not by the iteration: the landing of step t > 1 draws noise[T - t + 1]
 * wherever the loop was entered, noise[0] is read only when first_step == T,
 * and a loop entered at first_step < T reads rows T - first_step + 1 ..
 * T - max(last_step, 2) + 1 alone (the caller may pass the address row 0
 * would have without owning the rows before them).  quat_codes: NULL or
 * [n_iterations][B,N,N].  record: NULL or [n_iterations][B,N,3], x after
 * every iteration. */
int genie_sample_loop(genie_handle_t h, genie_stream_t stream, float scale,
                      const float* noise, const int8_t* quat_codes,
                      int first_step, int last_step,
                      float* trans_io, float* rots_io, float* record);

/* genie_p_sample in coefficient form, for a step from timestep t to any s < t and for either sampler:
 * trans <- ((a trans + bz z) * mask [+ c_scaled eps]) * mask, then Frenet frames.  eps == NULL: no noise (the last step).
 * genie_p_sample(step, scale) is a = 1/sqrt(alpha_t), bz = -w_z/sqrt(alpha_t), c_scaled = scale sqrt(beta_t); the rows of
 * pack.reverse_coefficients give (a, bz, C) for strided ancestral and DDIM steps, c_scaled = scale * C.
 * Returns GENIE_E_ARG, before anything is launched, for a NULL trans_inout, rots_out or z and for a non-finite coefficient. */
int genie_reverse_step(genie_handle_t h, genie_stream_t stream, float a, float bz, float c_scaled,
                       float* trans_inout, float* rots_out, const float* z, const float* eps /* NULL: no noise */);

/* genie_sample_loop over a sub-sequence of the timesteps, device resident (no host read): iteration i denoises at steps[i] and
 * applies genie_reverse_step with coef[i]; the last iteration draws no noise.  With start_from_noise the state starts as noise[0]
 * and its frames; without, trans_io / rots_io carry it in and noise[0] is not read (a resumed loop passes the tail of steps, coef,
 * noise and quat_codes, beginning one before the first remaining draw).
 * Returns GENIE_E_ARG, before anything is launched, with genie_last_error naming this entry: n_iter < 1; steps not strictly
 * decreasing or outside 1..n_timestep; NULL steps, coef, trans_io or rots_io; NULL noise when start_from_noise or n_iter > 1;
 * a non-finite coefficient. */
int genie_sample_loop_steps(genie_handle_t h, genie_stream_t stream, int n_iter,
                            const int32_t* steps /*host, strictly decreasing, in 1..T*/,
                            const float* coef /*host [n_iter][3]: a, bz, c_scaled*/,
                            const float* noise /*[n_iter][B,N,3]: noise[0] initial trans when start_from_noise, noise[k] the draw of iteration k-1's landing*/,
                            const int8_t* quat_codes /*NULL or [n_iter][B,N,N]*/, int start_from_noise,
                            float* trans_io, float* rots_io, float* record /*NULL or [n_iter][B,N,3]*/);

/* ---- arithmetic -------------------------------------------------------- */

/* How the pair-stack GEMMs (triangle multiplication, pair transition: 95 % of the FLOPs of
 * genie/model/model.py:125-192) are carried out.  Both give f32 results to the stated tolerance;
 * the reference computes them with f32 torch.matmul / nn.Linear.
 *   GENIE_MATH_HX  (default) every f32 operand is split in two f16 halves (22 significand bits) and
 *                  a product is three f16 MFMAs accumulated in f32 (csrc/hx.h);
 *   GENIE_MATH_F32 exact f32 MFMA (v_mfma_f32_32x32x2_f32), 1/16 of the matrix rate.
 * May be switched at any time between calls (both weight images are kept).  The environment
 * variable GENIE_MATH=f32|hx sets the initial mode of new handles. */
#define GENIE_MATH_F32 0
#define GENIE_MATH_HX 1
int genie_set_math(genie_handle_t h, int mode);
int genie_get_math(genie_handle_t h);

/* ---- training step (genie/diffusion/genie.py:60-120) ---------------------
 * The two ends around the denoiser first (noising, loss), then the optimizer and the forward + backward pass through the
 * Denoiser itself (genie_train_forward_backward).  All work on the batch bound with genie_prepare_features. */

/* Forward noising + frames (genie.py:80-87):
 *   trans_s = c_x0[b] x0 + c_z[b] z,   rots_s = compute_frenet_frames(trans_s)
 * with c_x0 = sqrt_alphas_cumprod[s], c_z = sqrt_one_minus_alphas_cumprod[s] (device, [B]; ddpm.py:54-56) and z
 * already masked by the caller (genie.py:77). */
int genie_q_sample(genie_handle_t h, genie_stream_t stream, const float* x0 /*[B,N,3]*/, const float* z /*[B,N,3]*/,
                   const float* c_x0 /*[B]*/, const float* c_z /*[B]*/, float* trans_out /*[B,N,3]*/,
                   float* rots_out /*[B,N,3,3]*/);

/* The loss training_step returns (genie.py:90-105, utils/loss.py:4-36) and its gradient:
 *   losses_out (device) [2 + 2B] = unweighted_loss, weighted_loss, condition_losses[B], infill_losses[B];
 *   grad_out [B,N,3] = d weighted_loss / d z_pred, or NULL.
 * Masks are the bound batch's residue_mask and fixed_sequence_mask; num_residues is taken as the mask's
 * row sum (feat_utils.py:17-65 builds them so). */
int genie_training_loss(genie_handle_t h, genie_stream_t stream, const float* z_pred /*[B,N,3]*/, const float* z /*[B,N,3]*/,
                        float condition_loss_weight, float* losses_out, float* grad_out);

/* One Adam update over a flat fp32 parameter blob (torch.optim.Adam as configured by ddpm.py:73-77: betas, eps,
 * no weight decay, no amsgrad), all arrays on the device, `step` = 1 for the first update; the scalars are doubles because
 * torch derives 1 - beta and the bias corrections in double before it rounds them:
 *   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps). */
int genie_adam_step(genie_stream_t stream, size_t n, float* p, const float* g, float* m, float* v, double lr, double beta1,
                    double beta2, double eps, int step);

/* The training step's forward and backward pass through the Denoiser (genie/diffusion/genie.py:88-105; what Lightning's
 * automatic optimisation runs between training_step and the optimizer, train.py:54-65), for the batch bound with
 * genie_prepare_features:
 *   output = Denoiser(T(rots, trans), timesteps, features)            (train mode: dropout live, see opts)
 *   loss   = the weighted loss of genie_training_loss(output['z'], z_target)
 *   grads  = d loss / d weights
 * `weights` and `grads` are DEVICE blobs owned by the caller in Denoiser.state_dict() order (the layout genie_load_weights takes
 * from the host; genie_weight_count floats): the optimizer (genie_adam_step) and the DDP gradient all-reduce (torch.distributed
 * over RCCL, train.py:57-59) act on them directly.  losses_out as genie_training_loss; z_pred_out [B,N,3] optional.
 * Dropout (modules/dropout.py:23-76 row-shared on both triangle multiplications, rate tri_dropout; nn.Dropout on s + ipa(s) and
 * inside StructureTransition, structure_net.py:109, structure_transition.py:66) uses counter-based masks derived from `seed`;
 * train_mode = 0 gives the eval-mode forward (what tests/golden/train_grads_n16_b2.npz was recorded in).
 * fast_math: how the GEMMs' f32 operands reach the bf16 matrix pipe -- 0: split in three bf16 pieces (24 significand bits, six MFMAs
 * per product: f32-grade -- the reference's arithmetic, its Trainer sets no `precision=` (train.py:54-65) and trains in fp32; the
 * mode every parity test and every quoted figure uses), 2: two pieces (16 bits, three MFMAs), 1: plain bf16 operands (one MFMA;
 * what a bf16-autocast run would compute -- NARROWER than the reference, offered for BASELINE config 5's "bf16" wording only).
 * A handle with n_head_tri > 0 is refused with GENIE_E_ARG ("triangular attention: ..."): the backward pass through the
 * attention is not built; the same holds for genie_denoise_vjp. */
typedef struct {
    float tri_dropout, ipa_dropout, transition_dropout;
    uint32_t seed;
    int32_t train_mode, fast_math;
    void* struct_done_event;   /* hipEvent_t or NULL: recorded on `stream` once the gradients of every structure_net.* tensor (the tail
                                  of the blob) are final, so that their all-reduce can overlap the pair stack's backward pass */
} genie_train_opts_t;
int genie_train_forward_backward(genie_handle_t h, genie_stream_t stream, const float* weights, float* grads, const float* trans /*[B,N,3]*/,
                                 const float* rots /*[B,N,3,3]*/, const int32_t* timesteps /*[B]*/, const float* z_target /*[B,N,3]*/,
                                 const int8_t* quat_codes /*[B,N,N] or NULL*/, float condition_loss_weight, const genie_train_opts_t* opts,
                                 float* losses_out /*[2 + 2B]*/, float* z_pred_out);
/* Vector-Jacobian product of the denoiser wrt its input translations, frames held fixed: what the fork's twisted-diffusion / SMC
 * samplers take with torch.autograd.grad(log_prob, ts.trans) after ts = T(rots.detach(), trans.detach())
 * (genie/sampler/unconditional_smc.py:465-482, 570-576):
 *   z_out      [B,N,3] = Denoiser(T(rots, trans), timesteps, features)['z']   (eval mode; may be NULL)
 *   dtrans_out [B,N,3] = sum over z entries of dz * d z / d trans
 * through the direct term, the frame translations entering the structure net and every IPA layer, and the template distance
 * bins of the pair feature net.  `weights`: device blob as for genie_train_forward_backward.  No weight gradients are formed. */
int genie_denoise_vjp(genie_handle_t h, genie_stream_t stream, const float* weights, const float* trans, const float* rots,
                      const int32_t* timesteps, const int8_t* quat_codes, const float* dz, float* z_out, float* dtrans_out);
/* Bytes of activations + scratch the last training call holds; the kept-for-backward part alone; the algorithmic FLOP (2 M N K per
 * product) of the GEMMs the last genie_train_forward_backward launched (bench.py's train_step leg prices them with it). */
size_t genie_train_workspace_bytes(genie_handle_t h);
size_t genie_train_kept_bytes(genie_handle_t h);
double genie_train_gemm_flop(genie_handle_t h);

/* The training path's building block, exposed so that it can be checked on its own (tests/test_train_gemm.py; the reference has no
 * counterpart: there these are torch.nn.Linear / einsum calls inside autograd, the files under genie/model).  Device pointers, element strides:
 *   C[z][m][n] (op)= alpha * sum_k A[z][m][k] B[z][k][n] (+ bias[n]),   z = z1 * nb2 + z2,  z1 < batch / nb2
 *   A at a + z1 a1 + z2 a2 + m am + k ak;  B at b + z1 b1 + z2 b2 + k bk + n bn;  C at c + z1 c1 + z2 c2 + m cm + n cn
 * mode 0 store (then optionally relu, and / or zero where gate <= 0, gate laid out like C), 1 add, 2 atomic add (required for
 * nsplit > 1 or batches sharing C).  terms: bf16 pieces per f32 operand (1 = bf16 products, 2 = 16 bits, 3 = f32-grade).
 * asum (optional, batch 1, am == 1, ak == M): asum[m] += sum_k A[m][k].
 * cblk > 0 (batch 1, at most 8 blocks): C is a row of separately placed blocks of cblk output rows (cblk_m = 1) or columns (0), block t
 * at c + ctab[t] with (m, n) at local index m - t cblk resp. n - t cblk, its asum entries at asum + atab[t] + local m -- how several
 * Linears sharing an input run as one GEMM (genie_train.hip lin_fwd_ln_cat / lin_bwd_w_ln_cat).  Returns 0, or -1 for an impossible shape. */
typedef struct {
    int32_t M, N, K, batch, nb2, nsplit, mode, terms, relu;
    int64_t am, ak, bk, bn, cm, cn, a1, a2, b1, b2, c1, c2;
    float alpha;
    int32_t cblk, cblk_m;
    int64_t ctab[8], atab[8];
} genie_gemm_desc_t;
int genie_train_gemm(genie_stream_t stream, const genie_gemm_desc_t* desc, const float* a, const float* b, float* c, const float* bias,
                     const float* gate, float* asum);

/* ---- measurement ------------------------------------------------------- */

/* Per-kernel-class HIP-event timing on the launch stream (bench.py roofline
 * leg).  enable != 0 starts recording (adds event overhead: not for timed
 * regions).  genie_profile_read synchronises and returns up to `cap` entries;
 * returns the number of classes, names are static strings. */
int genie_profile_enable(genie_handle_t h, int enable);
int genie_profile_read(genie_handle_t h, const char** names, double* total_ms,
                       int64_t* launches, int cap);

/* What dense f16 MFMA work the device sustains, measured live (csrc/probe_kernels.hip): the instruction stream of one transition stage
 * of the fused pair chain on every CU for about ms_target milliseconds (<= 0: 20 ms); synchronises.  The roofline is priced against
 * the datasheet peak (2.5 PFLOP/s dense f16); under matrix load the chip lowers its clock to its power budget and holds about
 * 1.3 - 1.7 PFLOP/s -- bench.py prints this number next to the kernels' own matrix rate.  No handle: nothing of the path calls it.
 * Returns 0 and TFLOP/s in *tflops_out (the launch's milliseconds in *ms_out if not NULL). */
int genie_probe_mfma(genie_stream_t stream, double ms_target, double* tflops_out, double* ms_out);

/* Workspace bytes currently held (HBM layout report for DESIGN.md). */
size_t genie_workspace_bytes(genie_handle_t h);

#ifdef __cplusplus
}
#endif
#endif
