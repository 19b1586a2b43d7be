/*
 * jamun_hip.h — C ABI of the MI355X-native JAMUN walk-jump sampling path.
 *
 * The reference (prescient-design/jamun) is pure Python and has no FFI of its own; its
 * extension points for this path are duck-typed Python protocols.  This header is the C ABI
 * that sits UNDER those protocols: each entry point names the reference interface it
 * replaces (paths relative to /root/reference).  Plain pointers and sizes only — no torch
 * types.  All device pointers are HIP device memory owned by the caller; all work is
 * enqueued on the `hipStream_t` passed in (as `void*`), with no internal synchronisation
 * unless stated.  Every function returns 0 on success or a negative error code; the message
 * is available from jamun_last_error() (thread-local).
 *
 * Build: hipcc --offload-arch=gfx950 -shared -fPIC (see jamun_amd/csrc/build.py).
 */
#ifndef JAMUN_HIP_H
#define JAMUN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JAMUN_OK 0
#define JAMUN_ERR_INVALID -1   /* bad argument / unsupported configuration */
#define JAMUN_ERR_MISSING -2   /* a required checkpoint tensor is missing  */
#define JAMUN_ERR_HIP -3       /* a HIP runtime call failed                */

/* A named host tensor in the reference's state-dict layout (fp32, contiguous).
 * Names are the reference's parameter names WITHOUT the "g." / "g._orig_mod." prefix,
 * e.g. "layers.3.gated_conv.f.f.radial_nn.3.weight"  (src/jamun/model/arch/e3conv.py:15-85,
 * src/jamun/e3tools/nn/_conv.py:76-92). */
typedef struct jamun_tensor {
  const char* name;
  const float* data; /* host pointer */
  int64_t numel;
} jamun_tensor;

/* Architecture + denoiser hyper-parameters
 * (src/jamun/hydra_config/model/arch/e3conv.yaml:3-14, src/jamun/model/denoiser.py:16-33). */
typedef struct jamun_hparams {
  int32_t n_layers;               /* hidden ConvBlocks (5)                       */
  int32_t mul0, mul1;             /* irreps_hidden = mul0 x0e + mul1 x1e (120,32) */
  int32_t edge_attr_dim;          /* 64: 32 bonded-embedding + 32 radial          */
  int32_t emb_dim[4];             /* atom_type, atom_code, residue_code, residue_index (8,8,32,8) */
  int32_t emb_rows[4];            /* embedding table rows (20,10,25,10)           */
  int32_t use_residue_sequence_index; /* 0: index zeroed (atom_embedding.py:69-71) */
  int32_t mean_center;            /* Denoiser.mean_center                         */
  float max_radius;               /* Denoiser.max_radius                          */
  float average_squared_distance; /* Denoiser.average_squared_distance            */
  float act_scalar_const;         /* e3nn normalize2mom(LeakyReLU(0.01))  = 1.4162684 */
  float act_gate_const;           /* e3nn normalize2mom(sigmoid)          = 1.8467055 */
  float w3j_111_sign;             /* +1: wigner_3j(1,1,1) = +eps/sqrt(6) (e3nn 0.5.4)   */
  int32_t separable;              /* hidden_layer_factory.conv: 0 jamun.e3tools.nn.Conv (e3conv.yaml), 1 SeparableConv
                                     (e3conv_separable.yaml; src/jamun/e3tools/nn/_conv.py:122-135, _tensor_product.py:8-58):
                                     expects <block>.gated_conv.f.f.tp.lin.weight and a radial_nn.3 of 2 n0 + 3 n1 rows */
} jamun_hparams;

/* Static description of the walker batch — what torch_geometric's Batch.from_data_list gives the
 * reference (src/jamun/cmdline/sample.py:27-38, src/jamun/utils/data_with_residue_info.py:17-33).
 * All host pointers.  bonds are directed pairs (src,dst) already offset into the batch. */
typedef struct jamun_topology {
  int32_t n_atoms;
  int32_t n_graphs;
  const int32_t* ptr;                    /* [n_graphs+1] first atom of each walker */
  const int32_t* atom_type_index;        /* [n_atoms] */
  const int32_t* atom_code_index;        /* [n_atoms] */
  const int32_t* residue_code_index;     /* [n_atoms] */
  const int32_t* residue_sequence_index; /* [n_atoms] */
  int32_t n_bonds;
  const int64_t* bond_src;               /* [n_bonds] edge_index[0] of the dataset's bonded edges */
  const int64_t* bond_dst;               /* [n_bonds] edge_index[1]                               */
} jamun_topology;

/* Langevin splitting-integrator parameters — the fields of the BAOAB/ABOBA dataclasses
 * (src/jamun/sampling/mcmc/_splitting.py:11-58) consumed by
 * src/jamun/sampling/mcmc/functional/_splitting.py:44-178. */
typedef struct jamun_mcmc_params {
  int32_t steps;              /* range(1, steps): steps-1 integrator iterations     */
  int32_t save_every_n_steps; /* >= 1                                               */
  int32_t burn_in_steps;
  int32_t has_clip;           /* 0: score_fn_clip = None                            */
  float delta, friction, M, inverse_temperature, score_fn_clip;
} jamun_mcmc_params;

/* Kernel-selection switches of jamun_sampler_create.  NOT needed in production: NULL (or all zero) selects the default kernels, and the
 * library reads no environment variables — these exist so that tests can run every implementation of a block against the others
 * (tests/test_gpu_parity.py) and profiling scripts can time an alternative.  Each field only EXCLUDES a kernel; what then runs is
 * reported by jamun_sampler_stats (conv_path / dg_mode / init_path / dg_emu). */
typedef struct jamun_tuning {
  int32_t no_dg;        /* hidden layers and initial projector on the general kernel k_conv (no destination-grouped tile plan)     */
  int32_t no_mf;        /* hidden layers: not k_conv_mf (A operand formed on the matrix cores); k_conv_dg (vector-ALU forming)      */
  int32_t dg_fp32;      /* k_conv_dg with v_mfma_f32_32x32x2_f32 instead of the f16x3 scheme (implies no_mf)                        */
  int32_t dg_no_alt;    /* k_conv_dg: not mode 1 (two passes over the hidden units for molecules above ~80 atoms)                   */
  int32_t dg_no_sp;     /* k_conv_dg: not mode 2 (single phase, spans up to ~52 atoms)                                              */
  int32_t dg_no_sph;    /* k_conv_dg: not mode 3 (single phase with one Y tile, spans up to ~73 atoms)                              */
  int32_t no_mfi;       /* initial projector: not k_conv_mfi / k_conv_mfx (matrix-core forming)                                      */
  int32_t no_init_v;    /* initial projector: not k_conv_init_v (edge by edge on the vector ALUs)                                    */
  int32_t node_fp32;    /* node update with v_mfma_f32_32x32x2_f32 (k_node_update) instead of f16x3 (k_node_update_h)                */
  int32_t edge_h_fp32;  /* radial MLP first layer with fp32 MFMAs (k_edge_h) instead of f16x3 (k_edge_h16)                           */
  int32_t dg_kgroups;   /* hidden-unit slices over XCD groups for the destination-grouped kernels: 0 (default = 1), 1, 2, 4, 8       */
  int32_t no_tail;      /* k_conv_mf: tiles with few destinations stay whole tiles (no k_tail_form / k_tail_contract)                 */
  int32_t no_short_k;   /* k_conv_mf: always four forming K-steps (64 source rows), also when every tile's sources fit the first 48      */
  int32_t no_ml;        /* hidden layers: not k_conv_ml (matrix-core forming for source spans of 63..167 atoms); k_conv_dg there              */
  int32_t seg_cost_tenths; /* work lists of the destination-grouped kernels: cost of a segment's prologue + epilogue in tenths of a (tile, hidden unit)
                              item when the lists are cut (0: the kernel's measured default — k_conv_mf 3.6, k_conv_ml 5.8 items —, -1: none)        */
  int32_t f16x1;        /* OPT-IN reduced precision of the hidden-layer conv (k_conv_mf / k_conv_ml): each fp32 product as ONE f16 MFMA (operands
                           rounded to 11 bits, fp32 accumulation) instead of the three of the f16x3 scheme; state, integrator, radial MLPs, initial
                           projector, node update and head stay as they are.  Never the default; x-hat then sits 2.5e-5 .. 7.6e-5 nm from the fp32
                           path on the test batches (asserted <= 1e-3 nm; the level of the reference's TF32 GPU path).  jamun_stats.dg_emu reports 2.  Ignored by the other conv kernels.   */
  int32_t no_fuse_geom; /* walks: k_finalize of an iteration and k_geom of the next as two launches instead of one (k_finalize_geom, round 6); A/B aid */
  int32_t selfcheck;    /* create-time self-check of the selected kernels against the general ones (one forward on synthetic positions through both;
                           node features after every block within 2e-5, else jamun_sampler_create returns JAMUN_ERR_INVALID): 0 / 1 on (default),
                           -1 off, 2 on with an injected fault in the selected conv kernel's weight stream (tests: the check must fire)   */
  int32_t no_tprod_t;   /* T pre-pass of k_conv_mf / k_conv_ml with k_tprod_h instead of k_tprod_t (round 6: weights through LDS, rows fetched whole,
                           transposed T stored as whole lines; bit-identical T); A/B aid                                                   */
} jamun_tuning;

typedef struct jamun_model jamun_model;     /* raw checkpoint tensors kept on the host          */
typedef struct jamun_sampler jamun_sampler; /* sigma- and topology-specific device state        */

const char* jamun_last_error(void);
int jamun_version(void);

/* Replaces Denoiser.load_from_checkpoint's module construction + load_state_dict
 * (src/jamun/hydra_config/model/denoiser_pretrained.yaml:1-2, src/jamun/model/denoiser.py:16-42). */
int jamun_model_create(const jamun_hparams* hp, const jamun_tensor* tensors, int32_t n_tensors, jamun_model** out);
void jamun_model_destroy(jamun_model* m);

/* Binds a model to one noise level and one walker batch: folds the noise-conditioning constants
 * (src/jamun/model/noise_conditioning.py:50-73), path normalisations and Clebsch-Gordan factors into
 * MFMA-ordered packed weights, uploads them, and allocates every work buffer.  Replaces
 * ModelSamplingWrapper.__init__ + the per-call graph clone (src/jamun/utils/sampling_wrapper.py:12-47).
 * Synchronous (uploads weights). */
int jamun_sampler_create(const jamun_model* m, float sigma, const jamun_topology* topo, const jamun_tuning* tuning /* NULL: defaults */,
                         jamun_sampler** out);
void jamun_sampler_destroy(jamun_sampler* s);

/* Denoiser.xhat (src/jamun/model/denoiser.py:203-217): y_dev [n_atoms,3] -> xhat_dev [n_atoms,3]. */
int jamun_xhat(jamun_sampler* s, const float* y_dev, float* xhat_dev, void* stream);
/* Denoiser.score (src/jamun/model/denoiser.py:111-114). */
int jamun_score(jamun_sampler* s, const float* y_dev, float* score_dev, void* stream);

/* baoab() (src/jamun/sampling/mcmc/functional/_splitting.py:112-178) with the model's score, fused with the
 * jump of SingleMeasurementSampler.walk_jump (src/jamun/sampling/walkjump/_single_measurement.py:49-79).
 *   y_dev, v_dev  [n_atoms,3]  in: y_init, v_init (already initialised) ; out: final y, v
 *   noise_dev     [steps-1, n_atoms, 3] standard-normal draws, one per iteration (reference RNG call order),
 *                 or NULL to draw them in-kernel from Philox4x32-10 keyed by (seed, iteration, atom)
 *   y_traj_dev, score_traj_dev, xhat_traj_dev  [T, n_atoms, 3] or NULL (save_trajectory=False);
 *                 T = jamun_num_frames(params, 0).  xhat_traj[t] = y_traj[t] + sigma^2 * score_traj[t]
 *                 (identical to the reference's extra forward per frame, in exact arithmetic).
 *                 With y_traj_dev == NULL (save_trajectory=False) a non-NULL score_traj_dev receives exactly ONE
 *                 frame, the initial score — the reference appends later scores only together with y
 *                 (_splitting.py:155,168-170) — so a [1, n_atoms, 3] buffer is enough and nothing past it is written.
 *   xhat_dev     [n_atoms,3] xhat(y_final) or NULL
 * No host synchronisation; all steps are enqueued on `stream`. */
int jamun_walk_baoab(jamun_sampler* s, float* y_dev, float* v_dev, const jamun_mcmc_params* p, const float* noise_dev,
                     uint64_t seed, float* y_traj_dev, float* score_traj_dev, float* xhat_traj_dev, float* xhat_dev,
                     void* stream);
/* aboba() (src/jamun/sampling/mcmc/functional/_splitting.py:44-109).  score_traj has T-1 frames (scores at the
 * half-step positions, :90,99-101); xhat_traj (if requested) costs one extra forward per saved frame, as the
 * reference (the half-step score cannot be reused). */
int jamun_walk_aboba(jamun_sampler* s, float* y_dev, float* v_dev, const jamun_mcmc_params* p, const float* noise_dev,
                     uint64_t seed, float* y_traj_dev, float* score_traj_dev, float* xhat_traj_dev, float* xhat_dev,
                     void* stream);
/* Number of saved y frames for (steps, save_every_n_steps, burn_in_steps); aboba's score_traj has one fewer
 * when burn_in_steps == 0.  */
int jamun_num_frames(const jamun_mcmc_params* p, int32_t* n_y_frames, int32_t* n_score_frames_baoab,
                     int32_t* n_score_frames_aboba);

/* ---- stand-alone operators of the path (also used for unit-level parity tests) -------------------------- */

/* mean_center (src/jamun/utils/mean_center.py:7-12): out = pos - centroid(graph).  ptr_dev [n_graphs+1] int32. */
int jamun_mean_center(const float* pos_dev, const int32_t* ptr_dev, int32_t n_graphs, float* out_dev, void* stream);

/* torch_geometric.nn.radius_graph(pos, r, batch) with torch_cluster CUDA semantics, call site
 * src/jamun/model/denoiser.py:149: per centre, scan its graph in index order, keep while d^2 < r^2 until 33 hits,
 * drop self.  Output is a fixed-stride neighbour table: nbr_dev [n_atoms, stride] (src indices, ascending),
 * deg_dev [n_atoms].  stride >= 33. */
int jamun_radius_graph(const float* pos_dev, const int32_t* ptr_dev, int32_t n_graphs, int32_t n_atoms, float r,
                       int32_t stride, int32_t* nbr_dev, int32_t* deg_dev, void* stream);

/* torch_scatter.scatter(src, index, dim=0, dim_size, reduce="mean"), call site src/jamun/e3tools/nn/_conv.py:117,
 * for a destination-sorted index given as CSR: rows seg_ptr[d]..seg_ptr[d+1] of src are averaged into out[d]
 * (empty segment -> 0).  Fixed summation order (row order), no atomics.  src_dev [E, width], out_dev [n_out, width]. */
int jamun_scatter_mean(const float* src_dev, const int32_t* seg_ptr_dev, int32_t n_out, int32_t width, float* out_dev,
                       void* stream);

/* One BAOAB iteration's state update around the score evaluation
 * (src/jamun/sampling/mcmc/functional/_splitting.py:158-166):
 *   pre : v += u*(delta/2)*psi ; y += (delta/2)*v ; vhat = exp(-gamma)*v + zeta*sqrt(u)*R ; y += (delta/2)*vhat
 *   post: psi = clip(score)*beta ; v = vhat + (delta/2)*psi          (no u, as the reference :166)
 * n = number of atoms; arrays are [n,3]. */
int jamun_baoab_pre(float* y_dev, float* v_dev, const float* psi_dev, const float* noise_dev, int32_t n,
                    const jamun_mcmc_params* p, void* stream);
int jamun_baoab_post(float* v_dev, float* psi_dev, const float* score_dev, int32_t n, const jamun_mcmc_params* p,
                     void* stream);

/* One ABOBA iteration's state update around the score evaluation
 * (src/jamun/sampling/mcmc/functional/_splitting.py:86-97):
 *   a : y += (delta/2)*v                                              (:87, the score is then evaluated at this y)
 *   b : psi = clip(score)*beta ; v += u*(delta/2)*psi ; vhat = exp(-gamma)*v + zeta*sqrt(u)*R ;
 *       v = vhat + (delta/2)*psi (no u, :96) ; y += (delta/2)*v
 * n = number of atoms; arrays are [n,3]. */
int jamun_aboba_a(float* y_dev, const float* v_dev, int32_t n, const jamun_mcmc_params* p, void* stream);
int jamun_aboba_b(float* y_dev, float* v_dev, const float* score_dev, const float* noise_dev, int32_t n,
                  const jamun_mcmc_params* p, void* stream);

/* Edge geometry of E3Conv.forward (src/jamun/model/arch/e3conv.py:114-123) for an explicit edge list: per edge e = (src -> dst),
 * from positions ALREADY scaled by c_in (as E3Conv receives them, src/jamun/model/denoiser.py:198):
 *   sh_dev     [n_edges, 4]        o3.SphericalHarmonics("1x0e+1x1e", normalize=True, normalization="component") = [1, sqrt(3) v/|v|]
 *   radial_dev [n_edges, n_basis]  e3nn soft_one_hot_linspace(|v|, 0, radial_cutoff, n_basis, basis="gaussian", cutoff=True)
 * (the radial half of edge_attr; the bonded half is an embedding lookup).  src_dev / dst_dev: int64 device arrays (edge_index);
 * pos_dev is [n_atoms, 3]: an edge with an index outside [0, n_atoms) reads nothing and gets NaN outputs. */
int jamun_edge_geometry(const float* pos_dev, int32_t n_atoms, const int64_t* src_dev, const int64_t* dst_dev, int32_t n_edges,
                        float radial_cutoff, int32_t n_basis, float* sh_dev, float* radial_dev, void* stream);

/* e3nn o3.Linear on node features between irreps (in0 x0e + in1 x1e) and (out0 x0e + out1 x1e): the skip / self-interaction /
 * head Linears of the path (src/jamun/e3tools/nn/_interaction.py:23-24, _mlp.py:69,109).  w_dev: the flat e3nn weight
 * [in0 x out0 | in1 x out1] on the device (instruction order i_in outer, i_out inner; path normalisation 1/sqrt(fan_in) applied
 * here).  x_dev [n_atoms, in0 + 3 in1] -> out_dev [n_atoms, out0 + 3 out1], e3nn layout (channel-major, m fastest). */
int jamun_node_linear(const float* x_dev, int32_t n_atoms, int32_t in0, int32_t in1, int32_t out0, int32_t out1, const float* w_dev,
                      int64_t w_numel, float* out_dev, void* stream);

/* The noise of the walks when noise_dev == NULL — the in-kernel replacement of the reference's per-step torch.randn_like
 * (src/jamun/sampling/mcmc/functional/_splitting.py:161; iid N(0,1) per atom and component): out_dev [n, 3] = the draws R of
 * integrator iteration `iteration` (1 .. steps-1) for atoms first_atom .. first_atom + n - 1 of a rank's batch under `seed`.
 * Philox4x32-10 (Salmon et al., SC'11) with key = seed (low, high word), counter = (atom, iteration, 0x4a414d55, 0); the four
 * output words w0..w3 give u_i = (float(w_i) + 0.5) * 2^-32, R = (sqrt(-2 ln u0) cos 2 pi u1, sqrt(-2 ln u0) sin 2 pi u1,
 * sqrt(-2 ln u2) cos 2 pi u3) (Box-Muller).  jamun_walk_baoab / jamun_walk_aboba with noise_dev == NULL are bit-identical to the
 * same walk fed these draws as noise_dev. */
int jamun_philox_normal(float* out_dev, int32_t n, uint64_t seed, uint32_t iteration, uint32_t first_atom, void* stream);

/* ---- trajectory file encoders: device frames -> the bytes of jamun_amd/pdb.py's save_pdb / save_dcd --------------------------------
 * Frames are fp32 in nanometres, addressed as xyz_dev[frame * frame_stride + atom * atom_stride + component] (strides in floats), so a
 * contiguous [n, T, 3] chain (frame_stride 3, atom_stride 3 T) and a slice of a [T, sum N, 3] trajectory (frame_stride 3 sum N,
 * atom_stride 3) are both read in place.  Caller-owned buffers, work queued on `stream`, no synchronisation.
 *
 * PDB: one model is the line "MODEL        {t}\n" (t unpadded) followed by a body that is constant per molecule apart from the 3 x 8
 * coordinate characters of each atom (ATOM records, TER, CONECT block, ENDMDL).  body_dev [body_len] is that body as the host printed it
 * once (pdb.pdb_model_template) and coord_off_dev [n_atoms] the ascending byte offset of each atom's x field in it (y and z follow).  The
 * call writes models first_model .. first_model + n_frames - 1 back to back to out_dev; their exact size comes from the host-only
 * jamun_pdb_models_nbytes (no device call), which is also how the caller sizes out_dev.  Each coordinate is printed as Python's
 * f"{v:8.3f}" of v = fp32(x * 10).  A value that is not finite or needs more than 8 characters is written as "   0.000" and counted into
 * *unencodable_dev (which the caller zeroes): a non-zero count means the caller must write that file on the host path. */
int jamun_pdb_models_nbytes(int64_t body_len, int64_t first_model, int64_t n_frames, int64_t* nbytes);
int jamun_encode_pdb_models(const float* xyz_dev, int64_t frame_stride, int64_t atom_stride, int32_t n_atoms, int32_t n_frames, int64_t first_model,
                            const uint8_t* body_dev, int64_t body_len, const int32_t* coord_off_dev, uint8_t* out_dev, int64_t out_capacity,
                            uint32_t* unencodable_dev, void* stream);
/* DCD: per frame three Fortran records  int32 4 n_atoms | n_atoms x fp32 (coordinate * 10.0f, Angstrom) | int32 4 n_atoms  for X, Y, Z:
 * n_frames * 3 * (4 n_atoms + 8) bytes, the coordinate block of a CHARMM DCD file behind its header.  out_dev must be 4-byte aligned. */
int jamun_encode_dcd_frames(const float* xyz_dev, int64_t frame_stride, int64_t atom_stride, int32_t n_atoms, int32_t n_frames, uint8_t* out_dev,
                            int64_t out_capacity, void* stream);

/* ---- superposition: frames -> frames aligned on a reference structure, and their RMSD to it ---------------------------------------------
 * What mdtraj's Trajectory.superpose does per frame, on the device.  Frames are addressed as the encoders above address them (frame and
 * atom strides in floats, components adjacent), input and output with their own strides; ref_dev [n_atoms, 3] is contiguous.  For every
 * frame: out = R (x - centroid(x)) + centroid(ref) with the PROPER rotation R (det +1, never a reflection) that minimises
 * sum_i |out_i - ref_i|^2 (Horn's quaternion method), and rmsd_dev[frame] = sqrt(mean_i |out_i - ref_i|^2) computed from the values written.
 * rmsd_dev may be NULL.  out_dev may be xyz_dev itself if the strides are equal too (in place); any other overlap of the memory the two
 * views span is JAMUN_ERR_INVALID.  n_atoms == 1: out = ref, rmsd = 0.  Rank-deficient frames (two atoms, collinear atoms) get a rigid image
 * with the minimal RMSD; the rotation about the free axis is arbitrary.  A frame with a non-finite value yields a non-finite frame and rmsd
 * and leaves the other frames alone.  Caller-owned buffers, work queued on `stream`, no synchronisation, no allocation. */
int jamun_superpose_frames(const float* xyz_dev, int64_t frame_stride, int64_t atom_stride, int32_t n_atoms, int32_t n_frames, const float* ref_dev,
                           float* out_dev, int64_t out_frame_stride, int64_t out_atom_stride, float* rmsd_dev, void* stream);

/* ---- internal coordinates: frames -> distances, bond angles and dihedrals of listed atoms -------------------------------------------------
 * What mdtraj's compute_distances / compute_angles / compute_dihedrals (and so compute_phi / compute_psi / compute_chi*) give per frame, on
 * the device.  Frames are addressed as the encoders above address them (frame and atom strides in floats, components adjacent).  idx_dev
 * [n_feat][4] int32 is the feature table: the number of LEADING non-negative entries of a row decides the feature (the rest are -1):
 *   2  distance   |p1 - p0|  (nm)
 *   3  bond angle at p1   atan2(|a x b|, a.b), a = p0 - p1, b = p2 - p1, in [0, pi]
 *   4  dihedral   b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, c1 = b2 x b3, c2 = b1 x b2: atan2((b1.c1) |b2|, c1.c2) in (-pi, pi] (IUPAC sign)
 *   0 or 1, or any of the leading entries >= n_atoms: NaN; such a row reads nothing.
 * out_dev is contiguous fp32 [n_frames][W]:
 *   cossin == 0   W = n_feat:    out[t][j] = the value of feature j in frame t
 *   cossin != 0   W = 2 n_feat:  out[t][2 j] = cos, out[t][2 j + 1] = sin of feature j's angle or dihedral, taken from the two atan2 arguments
 *                                (x, y) / |(x, y)| (not cos(atan2(..)): continuous across +-pi); a distance gives (d, 0), a NaN feature (NaN, NaN).
 * fp32 throughout, the differences formed first.  A non-finite coordinate makes exactly the features that use its atom in its frame NaN;
 * every other value is bit for bit what it is without it.  Degenerate geometry (coincident atoms, a collinear triple inside a dihedral) gives
 * what atan2f gives for the rounded arguments (atan2f(0, +-0) = 0 or pi; cos / sin = (+-1, 0)): finite for finite coordinates below 1e9 nm.
 * out_capacity (in floats) below n_frames * W is JAMUN_ERR_INVALID and nothing is written; n_feat == 0 or n_frames == 0 launches nothing and
 * succeeds.  Caller-owned buffers, work queued on `stream`, no synchronisation, no allocation. */
int jamun_internal_coords(const float* xyz_dev, int64_t frame_stride, int64_t atom_stride, int32_t n_atoms, int32_t n_frames,
                          const int32_t* idx_dev, int32_t n_feat, int32_t cossin, float* out_dev, int64_t out_capacity, void* stream);

/* ---- histograms of pairs of angle columns (Ramachandran plots) and their Jensen-Shannon divergence ----------------------------------------
 * angles_dev is fp32 [n_frames] rows of `width` values, row_stride floats apart (what the entry above writes: row_stride = width).
 * pairs_dev [n_pairs][2] int32 names the x and the y column of each histogram; edges_dev [bins + 1] fp64 holds the bin edges, ascending
 * (numpy's linspace(-pi, pi, bins + 1) uploaded: the bins then are numpy's by construction); 1 <= bins <= 128.  `cuts` is a HOST array of
 * n_cuts (1..64) frame counts, strictly ascending within [1, n_frames]; it is read before the call returns.  SEGMENT c holds the frames
 * cuts[c-1] <= t < cuts[c] (cuts[-1] := 0):
 *   counts_dev  uint32 [n_cuts][n_pairs][bins * bins]   bin (bx, by) at bx * bins + by: the frames of segment c whose (x, y) lie there.
 *                                                        The value, promoted to fp64, is clipped to [edges[0], edges[bins]] first; its bin is
 *                                                        the largest b <= bins - 1 with edges[b] <= value (the last edge is inclusive).
 *   skipped_dev uint32 [n_cuts][n_pairs]                 the frames of segment c whose x or y is not finite; they are in no bin.
 * Both outputs are zeroed by the call (on `stream`), so counts + skipped of a segment and pair add up to the segment's frames; a pair with
 * a column outside [0, width) counts nothing (skipped included) and reads nothing.  Integer atomic adds: the result is exact and the same
 * in every run.  counts_capacity (in counters) below n_cuts * n_pairs * bins * bins is JAMUN_ERR_INVALID, as is
 * every argument outside the ranges above, and then nothing is written; n_pairs == 0 launches nothing and succeeds.
 *
 * The second entry turns such segment counts into the curve "divergence from a reference against the number of frames": for every cut c the
 * PREFIX histogram (segments 0..c summed, uint64) is normalised and compared with the normalised reference ref_dev uint32
 * [n_ref_pairs][bins * bins], n_ref_pairs = n_pairs or 1 (one reference for every pair):
 *   per_pair_dev fp64 [n_cuts][n_pairs]   JSD(p, q) = (sum p log(p / m) + sum q log(q / m)) / 2, m = (p + q) / 2, in nats, 0 log 0 = 0
 *   pooled_dev   fp64 [n_cuts]            the same with all pairs (and all reference pairs) summed into one histogram first
 * fp64 throughout, summed in a fixed order: the value depends on the inputs alone.  A prefix or a reference without a count gives NaN.
 * Caller-owned buffers, work queued on `stream`, no synchronisation, no allocation. */
int jamun_hist2d_pairs(const float* angles_dev, int64_t row_stride, int32_t n_frames, int32_t width, const int32_t* pairs_dev, int32_t n_pairs,
                       const double* edges_dev, int32_t bins, const int32_t* cuts, int32_t n_cuts, uint32_t* counts_dev,
                       int64_t counts_capacity, uint32_t* skipped_dev, void* stream);
int jamun_js_divergence(const uint32_t* counts_dev, int32_t n_cuts, int32_t n_pairs, int32_t bins, const uint32_t* ref_dev, int32_t n_ref_pairs,
                        double* pooled_dev, double* per_pair_dev, void* stream);

/* ---- chemical validity: clashing non-bonded pairs and bonds of a wrong length, per frame ---------------------------------------------------
 * What the reference's metrics/_chemical_validity.py counts (_check_volume_exclusion, _check_bond_lengths), for every frame, on the device.
 * Frames are addressed as the encoders above address them (frame and atom strides in floats, components adjacent); 1 <= n_atoms <= 256.
 * For a pair (i, j) the number compared is s = (dx dx + dy dy) + dz dz, dx = x_j - x_i, every operation in fp32 in this order:
 *   clash_s_dev   fp32 [n_atoms (n_atoms - 1) / 2]  one threshold per pair i < j, the upper triangle in row-major order; the pair clashes when
 *                                                   s < clash_s.  A bonded pair carries 0.  May be NULL when n_atoms == 1.
 *   bonds_dev     int32 [n_bonds][2]                the bonds; bond b is off when s < bond_lo_s_dev[b] or s > bond_hi_s_dev[b] (fp32 [n_bonds]).
 *                                                   A row with an index outside [0, n_atoms) is skipped and reads nothing.  All three may be
 *                                                   NULL when n_bonds == 0.
 *   counts_dev    uint32 [n_frames][2]              (clashes, bonds that are off) of every frame; written whole by the call.
 *   bond_frames_dev uint32 [n_bonds] or NULL        the number of frames in which bond b is off; zeroed by the call (on `stream`).
 * The thresholds are made on the host so that the comparisons are those of the reference on fl32(sqrt(s)) (jamun_amd/validity.py); the
 * kernel takes no square root and the counts equal a host's that does the same fp32 operations, integer for integer.  A NaN compares false:
 * no issue; s = +inf is a bond that is off and no clash.  n_atoms == 1 gives zeros.  n_atoms outside [1, 256], a negative count or stride,
 * counts_capacity (in counters) below 2 n_frames or a NULL pointer that is needed is JAMUN_ERR_INVALID and nothing is written;
 * n_frames == 0 launches nothing and succeeds.  Caller-owned buffers, work queued on `stream`, no synchronisation, no allocation. */
int jamun_validity_counts(const float* xyz_dev, int64_t frame_stride, int64_t atom_stride, int32_t n_atoms, int32_t n_frames,
                          const float* clash_s_dev, const int32_t* bonds_dev, const float* bond_lo_s_dev, const float* bond_hi_s_dev,
                          int32_t n_bonds, uint32_t* counts_dev, int64_t counts_capacity, uint32_t* bond_frames_dev, void* stream);

/* ---- TICA of feature trajectories: lagged second moments, projection on fitted components, autocovariance sums -----------------------------
 * The three reductions over frames behind pyemma's tica(lag, kinetic_map) and statsmodels' acovf as the reference's analysis uses them
 * (analysis/utils.py: compute_TICA, compute_autocorrelation_stats); the fit itself (two symmetric eigenproblems of size width) is the
 * host's (jamun_amd/tica.py).  x_dev is fp32 [n_frames] rows of `width` values, row_stride floats apart (what jamun_internal_coords writes
 * with cossin: row_stride = width); 1 <= width <= 128, row_stride >= width; nothing is read behind the `width` values of a row.
 *
 * jamun_lagged_moments: for 1 <= lag < n_frames and the N = n_frames - lag pairs (x_t, x_{t+lag}), t < N, all fp64:
 *   sums_dev    [2][width]          sum_t x_t, then sum_t x_{t+lag}
 *   moments_dev [3][width][width]   G = sum_t x_t x_t^T, H = sum_t x_{t+lag} x_{t+lag}^T, K = sum_t x_t x_{t+lag}^T (row = the earlier
 *                                   frame; not symmetrised)
 * Every value is promoted to fp64 before it is multiplied, so every product is exact and the only rounding is in the additions: each
 * output is within gamma_N sum_t |a||b| of the exact sum (gamma_N = N u / (1 - N u), u = 2^-53).  The additions have a fixed order: the
 * pairs are cut into slices of 1024, a slice's terms are added in ascending t into work_dev [slices][2 width + 3 width^2], and the slices
 * are added in ascending order; no floating-point atomics.  The same inputs give the same bits in every run, and G and H are symmetric
 * bit for bit.  Non-finite inputs propagate by IEEE rules.  jamun_lagged_moments_work gives the size of the workspace in doubles
 * (0 for n_frames == 0); its contents before the call do not matter and mean nothing after it.
 *
 * jamun_project_frames: mean_dev fp64 [width], v_dev fp64 [width][d], 1 <= d <= width -> out_dev fp64 [n_frames][d],
 *   out[t][k] = sum_j (x[t][j] - mean[j]) v[j][k]
 * the difference formed in fp64, j ascending, one accumulator per output (within gamma_{width+1} sum_j |x - mean||v| of the exact value).
 * A non-finite x[t][j] makes exactly the d outputs of row t non-finite; every other row is bit for bit what it is without it.
 *
 * jamun_autocov_sums: y_dev fp64 [n_frames], `stride` (>= 1) doubles apart (column 0 of a projection is read in place: stride = d),
 * 0 <= max_lag <= 4096 -> out_dev fp64 [max_lag + 1],
 *   out[k] = sum_{t < n_frames - k} y_t y_{t+k},   0 for k >= n_frames
 * in fp64 (within gamma_{n_frames+1} sum_t |y_t y_{t+k}|), in the same fixed order as the moments (slices of 1024 values of t, workspace
 * [slices][max_lag + 1] doubles, jamun_autocov_sums_work).  The caller divides by n_frames - k: statsmodels' acovf(adjusted=True,
 * demean=False).  A product is formed only for t + k < n_frames.
 *
 * A negative count, stride or capacity, width outside [1, 128], lag outside [1, n_frames), d outside [1, width], max_lag outside [0, 4096],
 * row_stride < width, stride < 1, work_capacity or out_capacity (in doubles) below the need, or a NULL pointer is JAMUN_ERR_INVALID and
 * nothing is written; n_frames == 0 launches nothing, writes nothing and succeeds (the ranges of width, d and max_lag are checked first).
 * Caller-owned buffers, work queued on `stream`, no synchronisation, no allocation. */
int jamun_lagged_moments_work(int32_t n_frames, int32_t width, int32_t lag, int64_t* n_doubles);
int jamun_lagged_moments(const float* x_dev, int64_t row_stride, int32_t n_frames, int32_t width, int32_t lag, double* sums_dev, double* moments_dev,
                         double* work_dev, int64_t work_capacity, void* stream);
int jamun_project_frames(const float* x_dev, int64_t row_stride, int32_t n_frames, int32_t width, const double* mean_dev, const double* v_dev, int32_t d,
                         double* out_dev, int64_t out_capacity, void* stream);
int jamun_autocov_sums_work(int32_t n_frames, int32_t max_lag, int64_t* n_doubles);
int jamun_autocov_sums(const double* y_dev, int64_t stride, int32_t n_frames, int32_t max_lag, double* out_dev, double* work_dev, int64_t work_capacity,
                       void* stream);

/* ---- k-means and Markov state model counts of a projected trajectory (jamun_msm.hip) --------------------------------------------------------
 * The reductions over frames behind the reference's compute_MSM_stats (analysis/utils.py: pyemma's k-means, Markov state model and PCCA+);
 * Lloyd's loop, the estimators and PCCA are the host's (jamun_amd/msm.py).  y_dev is fp64 [n_frames] rows of d values, row_stride (>= d)
 * doubles apart: the output of jamun_project_frames, read in place.  1 <= k <= 1024, 1 <= d <= 128, k d <= 16384, 1 <= n_states <= 1024.
 *
 * jamun_assign_centers: centers_dev fp64 [k][d] (finite) -> labels_dev int32 [n_frames], the centre of smallest squared distance, the
 * lowest index on a tie.  The distance is  acc = +0.0;  for j ascending:  diff = y[j] - c[j];  sq = diff * diff;  acc = acc + sq  with
 * each of the three operations rounded on its own (no fused multiply-add), so label and distance equal the numpy loop of
 * msm.assign_centers_host bit for bit.  sqdist_dev (fp64 [n_frames], or NULL) receives the distance to the chosen centre.  A row with a
 * non-finite value gets label -1 and sqdist NaN; no other row is touched by it.  prev_labels_dev (int32 [n_frames]) and n_changed_dev
 * (one int64, ZEROED BY THE CALLER) go together or are both NULL: the number of frames whose label differs from prev_labels_dev is
 * ADDED to *n_changed_dev by integer atomics.  prev_labels_dev may be labels_dev itself.
 *
 * jamun_cluster_sums: labels_dev int32 [n_frames] -> counts_dev int64 [k], the rows that carry each label, and sums_dev fp64 [k][d], their
 * sum.  Labels outside [0, k) are skipped (-1 included).  Additions only, in a fixed order: the frames are cut into slices of 1024; within
 * a slice a cluster's rows are added in ascending frame order onto +0.0 (work_dev [slices][k d + k] doubles, jamun_cluster_sums_work); the
 * slices are added in ascending order onto +0.0.  msm.cluster_sums_host adds in the same order: the result equals it bit for bit and is
 * the same in every run.  With d = 1 on the sqdist of jamun_assign_centers it gives the inertia of every cluster.
 *
 * jamun_transition_counts: labels_dev int32 [n_frames], lag >= 1, map_dev int32 [n_in] or NULL -> counts_dev int64 [n_states][n_states],
 * ZEROED BY THE CALLER: counts[a][b] is INCREASED by the number of t < n_frames - lag with state(t) = a and state(t + lag) = b (sliding
 * counts; the counts of several chains add up and no pair crosses from one chain into the next).  state(t) is map[label] with a map
 * (n_in >= 1 entries, -1 for none) and the label itself without one (n_in is then ignored and taken as n_states); a pair is skipped when
 * a label is negative or >= n_in, or a state is outside [0, n_states).  lag >= n_frames counts nothing and succeeds.
 *
 * jamun_label_counts: the same labels and map, bounds_dev int32 [n_seg + 1] (non-decreasing, within [0, n_frames]; 1 <= n_seg <= 4096) ->
 * counts_dev int64 [n_seg][n_states], ZEROED BY THE CALLER: counts[s][a] is INCREASED by the number of frames bounds[s] <= t < bounds[s+1]
 * in state a.  Frames before bounds[0] or from bounds[n_seg] on count nowhere; bounds that do not ascend give counts that mean nothing but
 * never a write outside the table.
 *
 * The counts are integer atomics: exact in any order of arrival.  No floating-point atomics.  A negative count or stride, k, d, k d,
 * n_states or n_seg outside its range, row_stride < d, lag < 1, n_in < 1 with a map, work_capacity (in doubles) below the need, one of
 * prev_labels_dev / n_changed_dev without the other, or a NULL pointer that is needed is JAMUN_ERR_INVALID and nothing is written;
 * n_frames == 0 launches nothing, writes nothing and succeeds (the ranges are checked first).  Caller-owned buffers, work queued on
 * `stream`, no synchronisation, no allocation. */
int jamun_assign_centers(const double* y_dev, int64_t row_stride, int32_t n_frames, int32_t d, const double* centers_dev, int32_t k,
                         int32_t* labels_dev, double* sqdist_dev, const int32_t* prev_labels_dev, int64_t* n_changed_dev, void* stream);
int jamun_cluster_sums_work(int32_t n_frames, int32_t d, int32_t k, int64_t* n_doubles);
int jamun_cluster_sums(const double* y_dev, int64_t row_stride, int32_t n_frames, int32_t d, const int32_t* labels_dev, int32_t k,
                       int64_t* counts_dev, double* sums_dev, double* work_dev, int64_t work_capacity, void* stream);
int jamun_transition_counts(const int32_t* labels_dev, int32_t n_frames, int32_t lag, const int32_t* map_dev, int32_t n_in, int32_t n_states,
                            int64_t* counts_dev, void* stream);
int jamun_label_counts(const int32_t* labels_dev, int32_t n_frames, const int32_t* map_dev, int32_t n_in, int32_t n_states,
                       const int32_t* bounds_dev, int32_t n_seg, int64_t* counts_dev, void* stream);

/* ---- sliced Wasserstein distance of two clouds of descriptors (jamun_swd.hip) ---------------------------------------------------------------
 * What the reference's compute_sliced_Wasserstein_distance_of_ramachandran (metrics/_ramachandran.py) gets from the `ot` package: both
 * clouds projected on n_proj directions, per direction the 1-D Wasserstein distance at p = 2 with uniform weights (the clouds may differ
 * in size), and (mean over directions of W2^2)^0.5, which the caller takes from the n_proj values.  jamun_amd/swd.py is the specification.
 * 1 <= width <= 128, 1 <= n_proj <= 64, every count of frames or keys >= 1.
 *
 * jamun_swd_project: x_dev fp32 [n_frames] rows of `width` values, row_stride (>= width) floats apart, proj_dev fp32 [width][n_proj] ->
 * out_dev fp32 [n_proj][n_frames],  out[l][t] = fl32(sum_j double(x[t][j]) * double(proj[j][l])),  the sum in fp64 onto +0.0 with j
 * ascending, rounded to fp32 once.  A product of two promoted fp32 values is exact in fp64, so a fused and an unfused accumulate give the
 * same bits: the result equals swd.project_host bit for bit.
 *
 * "Sorted" below means sorted by the order image of swd.order_image (fp32 -> uint32: all bits of a negative flipped, the sign bit of a
 * non-negative set, every NaN sent to 0xFFFFFFFF): -0.0 < +0.0, NaN last and written as the quiet NaN 0x7FC00000.  A sorted column is
 * unique as bits.
 *
 * jamun_swd_sort_segments: keys_dev fp32 [n_proj][n_frames] and 1 to 64 cuts (a HOST array, ascending strictly within [1, n_frames]) ->
 * out_dev fp32 [n_proj][n_frames]: of every column the frames cuts[c-1] <= t < cuts[c] (cuts[-1] := 0) sorted, each segment on its own;
 * frames from the last cut on are copied as they are.  OUT OF PLACE: tiles of 4096 keys are sorted in LDS, then merge-path passes
 * alternate between out_dev and work_dev (jamun_swd_sort_work floats: n_proj * n_frames when a segment is longer than a tile, else 0)
 * and end in out_dev.  out_dev may be keys_dev itself; work_dev may overlap neither.
 *
 * jamun_swd_merge: sorted a_dev [n_proj] rows of n keys, a_stride (>= n) floats apart, and b_dev [n_proj] rows of m keys likewise ->
 * out_dev fp32 [n_proj][n + m], sorted; n + m fits 31 bits.  The device code is that of the sort's merge pass.
 *
 * jamun_swd_w2sq: sorted u_dev (rows of n) and v_dev (rows of m) as above -> out_dev fp64 [n_proj], the integral over q in [0, 1] of
 * (F^-1(q) - G^-1(q))^2 for the two empirical quantile functions: on the grid of n m cells the overlaps of u's cell i (length m) and v's
 * cell j (length n) contribute  w * (double(u_i) - double(v_j))^2,  w the overlap's integer length, formed as a difference, a square and a
 * product, each rounded once; the sum is divided by double(n m).  The terms are added in a fixed order (work_dev: jamun_swd_w2sq_work
 * doubles), so the same inputs give the same bits in every run, within (n + m) 2^-52 relative of any other order.  A non-finite key makes
 * its own column's value non-finite and touches no other column.
 *
 * A count below 1, width or n_proj outside its range, cuts that do not ascend strictly within [1, n_frames], a row stride below the
 * row's length, n + m above 2^31 - 1, a capacity (in floats, or in doubles for jamun_swd_w2sq) below the need or a NULL pointer that is
 * needed is JAMUN_ERR_INVALID and nothing is written.  Caller-owned buffers, work queued on `stream`, no synchronisation, no allocation,
 * nothing read back. */
int jamun_swd_project(const float* x_dev, int64_t row_stride, int32_t n_frames, int32_t width, const float* proj_dev, int32_t n_proj, float* out_dev,
                      int64_t out_capacity, void* stream);
int jamun_swd_sort_work(int32_t n_frames, int32_t n_proj, const int32_t* cuts, int32_t n_cuts, int64_t* n_floats);
int jamun_swd_sort_segments(const float* keys_dev, int32_t n_frames, int32_t n_proj, const int32_t* cuts, int32_t n_cuts, float* out_dev,
                            int64_t out_capacity, float* work_dev, int64_t work_capacity, void* stream);
int jamun_swd_merge(const float* a_dev, int64_t a_stride, int32_t n, const float* b_dev, int64_t b_stride, int32_t m, int32_t n_proj, float* out_dev,
                    int64_t out_capacity, void* stream);
int jamun_swd_w2sq_work(int32_t n, int32_t m, int32_t n_proj, int64_t* n_doubles);
int jamun_swd_w2sq(const float* u_dev, int64_t u_stride, int32_t n, const float* v_dev, int64_t v_stride, int32_t m, int32_t n_proj, double* out_dev,
                   double* work_dev, int64_t work_capacity, void* stream);

/* ---- denoising evaluation: the two ends of Denoiser.noise_and_denoise / compute_loss around the forward -----------------------------------
 * (src/jamun/model/denoiser.py:219-297, utils/align.py:9-56.)  A ragged batch of n_graphs graphs and n_atoms atoms: ptr_dev [n_graphs + 1]
 * int32 on the device, the atoms of graph g are ptr[g] .. ptr[g + 1] - 1, as jamun_mean_center takes it.  The kernels clamp the table to
 * [0, n_atoms], so a table that does not ascend from 0 to n_atoms gives values that mean nothing but never an access outside the buffers.
 * One workgroup per graph, fp32, every product and sum rounded on its own, every sum in a fixed order: the same inputs give the same bits
 * in every run.  No floating-point atomics.
 *
 * jamun_noise_align_graphs   x_dev, noise_dev [n_atoms, 3] -> x_c_dev, y_dev [n_atoms, 3], rmsd_dev [n_graphs] (may be NULL):
 *     x_c = x - centroid(x)                      only if mean_center != 0, else x_c = x
 *     y   = x_c + sigma * noise
 *     y  -= centroid(y)                          only if mean_center != 0
 *     y   = R (y - c_y) + c_x                    only if align != 0: c_y, c_x the centroids of y and x_c, R the PROPER rotation (det +1, never
 *                                                a reflection) that minimises sum_i |R (y_i - c_y) + c_x - x_c,i|^2
 *     rmsd[g] = sqrt(mean_i |y_i - x_c,i|^2)     of the values written
 *   Every centroid is the sequential fp32 sum in atom order divided by the count: x_c holds the bits of jamun_mean_center(x), and without
 *   align y those of the same fp32 operations done on a host.  R is the top eigenvector of Horn's quaternion matrix of the covariance of the
 *   centred coordinates (cyclic Jacobi sweeps, as jamun_superpose_frames): graphs of one or two atoms or of collinear atoms get some optimal
 *   rotation and finite values, the mirror image of x gets the best rotation with rmsd > 0.  A graph with a non-finite value gets a
 *   non-finite y and leaves every other graph alone; a graph without atoms writes nothing (rmsd[g] included).  x_c_dev may be x_dev.
 *
 * jamun_denoise_loss   xhat_dev, x_c_dev [n_atoms, 3], loss_weight_dev [n_graphs] (NULL: ones) -> out_dev [n_graphs, 3]:
 *     out[g][0] = raw_coordinate_loss = mean_i |xhat_i - x_i|^2
 *     out[g][1] = scaled_rmsd         = mean_i |xhat_i - x_i| / (sigma * sqrt(3))
 *     out[g][2] = coordinate_loss     = out[g][0] * loss_weight[g] * inv_c_out_sq
 *   The per-atom terms of a graph are added in atom order in fp32, as scatter_mean adds them on the CPU; a graph without atoms gives zeros.
 *
 * A NULL pointer that is needed, a negative count, sigma that is not finite or not above 0, 3 n_atoms beyond 31 bits or a ptr_dev that is
 * not device memory is JAMUN_ERR_INVALID and nothing is written; n_graphs == 0 launches nothing.  Caller-owned buffers, work queued on
 * `stream`, no synchronisation, no allocation, nothing read back. */
int jamun_noise_align_graphs(const float* x_dev, const float* noise_dev, const int32_t* ptr_dev, int32_t n_graphs, int32_t n_atoms, float sigma,
                             int32_t mean_center, int32_t align, float* x_c_dev, float* y_dev, float* rmsd_dev, void* stream);
int jamun_denoise_loss(const float* xhat_dev, const float* x_c_dev, const int32_t* ptr_dev, int32_t n_graphs, int32_t n_atoms, float sigma,
                       const float* loss_weight_dev, float inv_c_out_sq, float* out_dev, void* stream);

/* The graph half of a forward on its own: Denoiser.add_edges + the edge geometry + the radial MLPs' hidden layer
 * (src/jamun/model/denoiser.py:138-166, arch/e3conv.py:110-127, e3tools/nn/_conv.py:112) for positions y_dev [n_atoms,3]; the
 * result stays inside the sampler as the edge table the blocks below run on. */
int jamun_build_edges(jamun_sampler* s, const float* y_dev, void* stream);

/* ONE block of E3Conv on caller-owned node features and the sampler's current edge table (jamun_build_edges, or the last forward):
 *   layer 0      x_out = ConvBlock_initial(noise-scaled atom embedding)                     x_in_dev must be NULL (the input is the
 *                                                                                           sampler's own constant embedding)
 *   layer l >= 1 x_out = w_l * x_in + (1 - w_l) * ConvBlock_l(s_l * x_in)                   x_in_dev [n_atoms, mul0 + 3 mul1]
 * i.e. ConvBlock = LinearSelfInteraction(Gated(Conv)) (src/jamun/e3tools/nn/_conv.py:147-221: gather, radial-MLP weights, tensor
 * product, scatter-mean, gate, self-interaction + skip Linear) with the noise-conditional scaling and skip of
 * src/jamun/model/arch/e3conv.py:129-133 around it.  x_out_dev [n_atoms, mul0 + 3 mul1]; must not alias x_in_dev. */
int jamun_conv_block(jamun_sampler* s, int32_t layer, const float* x_in_dev, float* x_out_dev, void* stream);

/* Introspection for tests / benchmarks. */
typedef struct jamun_stats {
  int64_t n_edges;        /* directed edges (radial + bonded) in the last forward             */
  int64_t flop_ref_assoc; /* FLOPs of one forward in the reference association (SURVEY §8 d)  */
  int64_t flop_executed;  /* FLOPs actually issued on MFMA/VALU by this implementation         */
  int64_t conv_k0, conv_k1; /* padded contraction depth of the scalar / vector conv GEMMs (hidden layer; H + 1 hidden rows, H = edge_attr_dim) */
  int64_t conv0_flop_alg;   /* useful FLOPs of ONE hidden-layer scalar-row conv launch: 2*n_atoms*(H+1)*(mul0+mul1)*(mul0+mul1) (H + 1 = 65 by default) */
  int64_t conv1_flop_alg;   /* useful FLOPs of ONE hidden-layer vector-row conv launch: 2*3*n_atoms*(H+1)*(mul0+2*mul1)*mul1   */
  int32_t edge_stride;
  int32_t n_slices;       /* partial slabs per tile summed by the node update (max over tiles)          */
  int32_t conv_path;      /* hidden layers: 3 the wide path (jamun_wide.hip: Conv models outside the compiled-width kernels' envelope — any
                             hidden width, edge_attr_dim != 64, embeddings above 224 channels; fp32 MFMAs, jamun_tuning.f16x1 ignored),
                             2 destination-grouped kernels on host-planned tiles (jamun_conv_mf.hip / jamun_conv_dg.hip),
                             0 general k_conv (any irreps, any topology; also SeparableConv's slot in this field) */
  int32_t dg_mode;        /* destination-grouped kernel: 5 jamun_conv_ml.hip (as 4, for source spans of 63..167 atoms: two passes over the hidden
                             units with the vector / scalar channels resident, block-sparse forming over the occupied 16-row source blocks);
                             4 jamun_conv_mf.hip (A operand formed on the matrix cores and chained into the
                             contraction; source spans up to 62 atoms); jamun_conv_dg.hip (A operand formed edge by edge on the vector ALUs):
                             0 two phases per hidden unit with resident source rows, 1 two passes over the hidden units (molecules above
                             ~80 atoms), 2 single phase (spans up to ~52 atoms), 3 single phase with one Y tile (spans up to ~73 atoms);
                             -1: not in use */
  int32_t init_path;      /* initial projector: 6 k_conv_wide (the wide path, conv_path 3), 5 k_conv_mlx (jamun_conv_ml.hip: as 4 on the dg_mode 5 tiles — source spans of 63..167 atoms, block-sparse forming),
                             4 k_conv_mfx (jamun_conv_mf.hip: aggregated operand formed on the matrix cores from the embedding
                             rows, as a hidden layer with 64 scalar channels; dg_mode 4 tiles, any number of distinct embedding rows),
                             3 k_conv_mfi (coefficient sums per distinct embedding row formed with a one-hot selector, contracted with the
                             input-times-weight table; dg_mode 4 tiles, <= 32 distinct rows),
                             2 edge-by-edge VALU kernel on the tiles of jamun_conv_dg.hip (jamun_conv_initv.hip),
                             0 the general kernel k_conv  (1 was the table kernel jamun_conv_init.hip, retired in round 4) */
  int32_t dg_row_blocks;  /* jamun_conv_dg.hip: 1 when some molecule exceeds the span budget and its sources are cut into row blocks */
  int32_t dg_emu;         /* hidden-layer conv arithmetic: 2 f16x1 (jamun_tuning.f16x1: one f16 MFMA per product; k_conv_mf / k_conv_ml only), 1 f16x3 (three v_mfma_f32_*_f16 per fp32 product, operands split hi + lo),
                             0 v_mfma_f32_32x32x2_f32 (jamun_tuning.dg_fp32; always on the wide path, conv_path 3); -1: not in use */
  int64_t conv_flop_exec_launch; /* matrix-core FLOPs EXECUTED by ONE launch of the hidden-layer conv kernel (k_conv_mf / k_conv_dg; padding,
                             structural zeros of the forming GEMMs and the three products of the f16x3 scheme included; the T pre-pass is
                             a separate launch and not counted); 0 when another conv path is in use */
  int64_t conv_flop_useful_launch; /* of those, what the destination-grouped association needs at the edge count of the last forward:
                             3 (f16x3) x [2 x 65 x n_atoms x (G0 K0 + 3 G1 K1) contraction + 2 x 65 x n_edges x (in0 + 15 in1) forming
                             (x0, dot, x1, cross and T term per edge)], no padding, no zero blocks */
  int32_t n_tail_tiles;   /* tiles of the dg_mode-4 plan that go through k_tail_form / k_tail_contract instead of k_conv_mf (0: none)            */
  int32_t n_tail;         /* ... and their destinations                                                                                   */
  int64_t conv_bytes_alg_launch;  /* algorithmic HBM bytes of that launch: h~ of the layer, T, the weight stream once, the feature
                             rows once, the partial slabs written */
  int32_t mf_nks;         /* k_conv_mf: forming K-steps of 16 source rows per product (4; 3 when every tile's sources fit 48 rows; 0: other kernel) */
  int32_t ml_window;      /* k_conv_ml (dg_mode 5): source rows of the instantiation in use (96, 128 or 168); 0: other kernel */
} jamun_stats;
/* Synchronises `stream`. */
int jamun_sampler_stats(jamun_sampler* s, jamun_stats* out, void* stream);
/* Synchronises `stream` and returns JAMUN_ERR_INVALID if a matrix-formed conv kernel flagged, in any forward enqueued so far, an edge table
 * its coefficient tiles cannot represent (more than three edges of one ordered pair; a source outside the tile's window: host plan and kernel
 * disagree).  The flag also surfaces, unsynchronised, at the next entry point after its copy landed; call this where the results are about to
 * be consumed (jamun_amd.sampling.Sampler does, once per batch). */
int jamun_sampler_check(jamun_sampler* s, void* stream);

/* Per-kernel-class timing with HIP events recorded on the launch stream around each launch of the forward
 * (bench.py's roofline leg).  enable(1) starts collecting; read() synchronises `stream`, returns the summed
 * elapsed milliseconds and launch count per class (arrays of JAMUN_PROF_NCLASS) and clears the collection. */
#define JAMUN_PROF_GEOM 0        /* centring + radius graph + edge geometry                         */
#define JAMUN_PROF_EDGE_H 1      /* radial-MLP hidden layer per edge                                */
#define JAMUN_PROF_CONV0_INIT 2  /* conv contraction, initial projector (fused path: all rows)        */
#define JAMUN_PROF_CONV1_INIT 3  /* conv contraction, vector-output rows, initial projector          */
#define JAMUN_PROF_CONV0 4       /* conv contraction, hidden layers (dominant; fused path: all rows)  */
#define JAMUN_PROF_CONV1 5       /* hidden layers: tail tiles (k_tail_form + k_tail_contract); general kernel: vector-output rows */
#define JAMUN_PROF_NODE 6        /* partial-slab reduce + gate + self/skip Linear + noise skip mix   */
#define JAMUN_PROF_HEAD 7        /* output head + xhat/score finalize                                */
#define JAMUN_PROF_TPROD 8       /* T pre-pass of a hidden layer (k_tprod / k_tprod_h), in front of the conv kernel */
#define JAMUN_PROF_NCLASS 9
/* on = 0: off; 1: every class; otherwise a mask with bit (c + 1) set for each class c to time (event records are not free:
 * timing all 16 launches of a forward costs ~4 % of a step, the dominant class alone ~1 %). */
int jamun_profile_enable(jamun_sampler* s, int32_t on);
/* Sample instead of timing every launch: only every `every`-th launch of each enabled class gets its two event records (every >= 1;
 * 1 = all, the default after jamun_sampler_create).  An event record sits between two launches of the stream and costs ~1.3 us of a
 * 0.87 ms step each: the five hidden-layer conv launches of every step timed = 3 % of the step (bench.py: 295 k against 304 k
 * conformations/s); a stride that is coprime to the launches of the class per forward still visits every layer. */
int jamun_profile_sample(jamun_sampler* s, int32_t every);
int jamun_profile_read(jamun_sampler* s, double* ms_total, int64_t* launches, void* stream);

/* Diagnostic builds only (-DJAMUN_STAMP): summed s_memtime cycles per phase of the fused conv kernel
 * {coefficient-tile write, barrier wait, forming MFMAs, main MFMAs}; synchronises the device and clears the counters. */
int jamun_debug_stamps(unsigned long long* out8);

/* Copy internal buffers out for layer-level parity tests (device->device on `stream`):
 *   what = 0: node features after block `layer` (0 = initial projector) [n_atoms, mul0+3*mul1]
 *   what = 1: in-degree (radial + bonded) as float [n_atoms]
 *   what = 2: network output g [n_atoms,3] (before c_skip/c_out)                          */
int jamun_debug_read(jamun_sampler* s, int32_t what, int32_t layer, float* out_dev, void* stream);

/* Work lists of the destination-grouped conv kernels (tests/test_plan.py, tests/test_gpu_plans.py).  Segment records are int4 pairs
 * {tile, partial slab, k_begin, k_end}, {k_extra (-1: none), ...}, [grid][max_segs][2]; padding records have tile = -1.
 *
 * Host only, no device calls: runs the planner of jamun_sampler_create on caller-given tiles — tile_atoms [n_tiles][2] {first atom, atoms},
 * tile_chunk [n_tiles] (destination chunk; tiles of one chunk number their slabs jointly), tile_weight [n_tiles] (>= 1), skip [n_tiles]
 * (NULL: none; non-zero: the tile is not on this plan) — with cus workgroups, ng hidden-unit slices (1, 2, 4, 8; cus % 8 == 0 above 1),
 * n_k >= ng hidden units and seg_cost (a segment's prologue + epilogue in items, 0..1000).  Writes max_segs, n_slabs, atom_nslab [n_atoms]
 * and, when segs_out is not NULL, the records (segs_capacity >= cus * max_segs * 8 int32 values, else JAMUN_ERR_INVALID with max_segs written). */
int jamun_debug_plan_segments(int32_t cus, int32_t ng, int32_t n_k, int32_t n_atoms, int32_t n_tiles, const int32_t* tile_atoms,
                              const int32_t* tile_chunk, int32_t n_chunks, const int64_t* tile_weight, const int8_t* skip, double seg_cost,
                              int32_t* segs_out, int64_t segs_capacity, int32_t* max_segs, int32_t* n_slabs, int32_t* atom_nslab);
/* Host only, no device calls: the kernel selection of jamun_sampler_create (tile plan, hidden-layer kernel, tail tiles, work lists, initial
 * projector) for a model's hyper-parameters, tuning switches (NULL: defaults) and topology on a device with `cus` compute units, with
 * n_uniq distinct embedding rows and what packing produced given by the caller: hidden [n_hidden] per hidden layer bit 0 / 1 / 2 = its
 * weights for k_conv_dg / the matrix-formed kernels / the tail tiles are present; layer0 [5] = {k_conv_init_v table, k_conv_mfi table, its
 * selector tiles (1, 2, 4), k_conv_mfx weights, 32-column tiles of the scalar outputs} of the initial projector.
 * out24 = {conv_path, dg_mode, init_path, dg_emu, dg_RS, edge stride S, n_tiles, span_max, row_blocks, n_tail_tiles, n_tail, tail_runs,
 *          init_tail, own_init_segs, mf_nks, ml_window, initv_nbuf, ng, seg_cost_tenths, max_segs, n_slabs, conv_flop_exec_launch,
 *          max_segs, n_slabs of the initial projector's own lists}, the enumerations as jamun_stats documents them (SeparableConv: -1) and
 * as the plan holds them (dg_mode 0 and mf_nks 4 also where no destination-grouped kernel runs).
 * which = -1: no list; 0..5 as jamun_debug_segments (records without the tile descriptor), 6: destination chunk per tile.  list_len
 * receives the list's int32 values; list may be NULL, else capacity >= list_len. */
int jamun_debug_select_kernels(const jamun_hparams* hp, const jamun_tuning* tuning, const jamun_topology* topo, int32_t cus, int32_t n_uniq,
                               int32_t have_atom_uid, int32_t n_hidden, const int32_t* hidden, const int32_t* layer0, int64_t* out24,
                               int32_t which, int32_t* list, int64_t capacity, int64_t* list_len);
/* The lists a sampler's kernels run, copied to the host (synchronous; the sampler needs a destination-grouped plan):
 *   which = 0: hidden layers' segment records (the second record carries the tile descriptor {k_extra, first atom, atoms | rows << 8, first row})
 *           1: the initial projector's own records (none when it runs list 0)     2: tail-tile records [n_tail_tiles] int4
 *           3: tile table [n_tiles] {first atom, atoms, first source row, end}    4 / 5: partial slabs per atom [n_atoms] of list 0 / 1
 * info[9] = {int32 values of the list, grid, max_segs, n_slabs, k-slices, n_k, n_tiles, segment cost in tenths, tail runs}; out may be NULL
 * (info only), else capacity >= info[0]. */
int jamun_debug_segments(jamun_sampler* s, int32_t which, int32_t* out, int64_t capacity, int32_t* info);

/* Device and pinned-host allocations the library holds in this process right now, over all samplers: their number and their bytes as
 * requested (tests/test_gpu_memory.py: both return to their earlier values after a destroy and after a failed create).  Host only. */
int jamun_debug_live_allocations(int64_t* count, int64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* JAMUN_HIP_H */
