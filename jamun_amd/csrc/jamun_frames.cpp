// jamun_frames.cpp — the C entries that encode or analyse frames of a trajectory and never touch a jamun_sampler: the PDB / DCD encoders
// (jamun_traj.hip), superposition (jamun_superpose.hip), internal coordinates (jamun_intcoord.hip), histograms of angle pairs with their
// Jensen-Shannon divergence (jamun_hist.hip), chemical validity (jamun_validity.hip), the reductions behind TICA: lagged moments,
// projection, autocovariance sums (jamun_tica.hip), and those behind k-means and the Markov state model: nearest centres, cluster sums,
// transition and occupancy counts (jamun_msm.hip), and the sliced Wasserstein distance: projection, segment sort, merge, quantile integral
// (jamun_swd.hip).  Every refusal is raised before any HIP call.
// The order of an entry's checks decides which message a caller with two faults sees, and the entries differ in it on purpose: where a
// shared check below would change an order or a text, the entry keeps a line of its own.  Every entry's checks read top to bottom.
// The shared checks: check_range (every "NAME V is outside [LO, HI]"), check_row_stride, require_capacity, parse_cuts (the cuts of the
// histograms and of the segment sort), check_tica_lag, check_centers, check_states, swd_columns.  tests/golden/frames_refusals.json pins
// the code and the text of every refusal that ends before a launch, and which of two faults is the one reported.
#include "jamun_host.h"

namespace {

// A [n_frames, n_atoms, 3] view of floats: any strides over frames and atoms, the three components adjacent
struct FramesView {
  const float* ptr;
  int64_t frame_stride, atom_stride;
  int32_t n_atoms, n_frames;
  bool negative() const { return frame_stride < 0 || atom_stride < 0 || n_atoms < 0 || n_frames < 0; }  // (a stride or a count)
  // floats spanned: one past the last component (n_frames, n_atoms >= 1)
  unsigned __int128 span() const {
    return (unsigned __int128)(n_frames - 1) * (unsigned __int128)frame_stride + (unsigned __int128)(n_atoms - 1) * (unsigned __int128)atom_stride + 3;
  }
};

void require_capacity(const char* name, int64_t have, int64_t need, const char* what, const char* unit) {
  if (have < need)
    throw Err(JAMUN_ERR_INVALID, std::string(name) + " " + std::to_string(have) + " is too small: the " + what + " need " + std::to_string(need) + " " + unit);
}

void check_range(const char* name, int64_t v, int64_t lo, int64_t hi) {
  if (v < lo || v > hi)
    throw Err(JAMUN_ERR_INVALID, std::string(name) + " " + std::to_string(v) + " is outside [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
}

// rows `stride` elements apart hold `width` adjacent ones; `what` words the width: "the width " or "d = "
void check_row_stride(int64_t stride, int32_t width, const char* what) {
  if (stride < width) throw Err(JAMUN_ERR_INVALID, "row_stride " + std::to_string(stride) + " is below " + what + std::to_string(width));
}

void check_tica_lag(int32_t lag, int32_t n_frames) {
  if (lag < 1 || lag >= n_frames)
    throw Err(JAMUN_ERR_INVALID, "lag " + std::to_string(lag) + " is outside [1, n_frames = " + std::to_string(n_frames) + ")");
}

void check_centers(int32_t k, int32_t d) {
  check_range("k", k, 1, JAMUN_MSM_MAX_K);
  check_range("d", d, 1, JAMUN_MSM_MAX_D);
  if ((int64_t)k * d > JAMUN_MSM_MAX_KD)
    throw Err(JAMUN_ERR_INVALID, "k * d = " + std::to_string((int64_t)k * d) + " is above " + std::to_string(JAMUN_MSM_MAX_KD));
}

// the states of a count table and the table the labels go through first; returns the number of labels taken
int32_t check_states(int32_t n_states, const int32_t* map_dev, int32_t n_in) {
  check_range("n_states", n_states, 1, JAMUN_MSM_MAX_STATES);
  if (map_dev && n_in < 1) throw Err(JAMUN_ERR_INVALID, "n_in " + std::to_string(n_in) + " is below 1: a map has at least one entry");
  return map_dev ? n_in : n_states;
}

// n_cuts cuts (a host array) ascending strictly within [1, n_frames], as the kernels take them: their number, the pointer, the ascent
JamunHistCuts parse_cuts(const int32_t* cuts, int32_t n_cuts, int32_t n_frames) {
  check_range("n_cuts", n_cuts, 1, JAMUN_HIST_MAX_CUTS);
  if (!cuts) throw Err(JAMUN_ERR_INVALID, "null argument");
  JamunHistCuts k;
  k.n = n_cuts;
  for (int c = 0; c < JAMUN_HIST_MAX_CUTS; ++c) k.cut[c] = c < n_cuts ? cuts[c] : 0;
  for (int c = 0; c < n_cuts; ++c)
    if (k.cut[c] < 1 || k.cut[c] > n_frames || (c > 0 && k.cut[c] <= k.cut[c - 1]))
      throw Err(JAMUN_ERR_INVALID, "cuts[" + std::to_string(c) + "] = " + std::to_string(k.cut[c]) + ": the cuts must ascend strictly within [1, " +
                                       std::to_string(n_frames) + "]");
  return k;
}

// the cuts of jamun_swd_sort_segments, behind the two counts they are checked against
JamunHistCuts swd_cuts(int32_t n_frames, int32_t n_proj, const int32_t* cuts, int32_t n_cuts) {
  check_range("n_frames", n_frames, 1, INT32_MAX);
  check_range("n_proj", n_proj, 1, JAMUN_SWD_MAX_PROJ);
  return parse_cuts(cuts, n_cuts, n_frames);
}

// two sets of n_proj sorted columns of n and m keys, their rows a_stride and b_stride floats apart
void swd_columns(int64_t a_stride, int32_t n, int64_t b_stride, int32_t m, int32_t n_proj) {
  check_range("n", n, 1, INT32_MAX);
  check_range("m", m, 1, INT32_MAX);
  check_range("n_proj", n_proj, 1, JAMUN_SWD_MAX_PROJ);
  if (a_stride < n || b_stride < m)
    throw Err(JAMUN_ERR_INVALID, "row strides " + std::to_string(a_stride) + " and " + std::to_string(b_stride) + " are below the lengths " +
                                     std::to_string(n) + " and " + std::to_string(m));
}

constexpr int64_t kMaxModel =1000000000000000ll;  // model numbers stay below 10^15 (16 digits: the MODEL line fits the kernel's header budget)

int64_t checked_pdb_nbytes(int64_t body_len, int64_t first_model, int64_t n_frames) {
  if (body_len < 0 || first_model < 0 || n_frames < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
  if (body_len > INT32_MAX) throw Err(JAMUN_ERR_INVALID, "body_len must fit 31 bits");
  if (first_model > kMaxModel || n_frames > kMaxModel) throw Err(JAMUN_ERR_INVALID, "model numbers must stay below 10^15");
  return pdb_models_nbytes(body_len, first_model, n_frames);
}

}  // namespace

extern "C" {

// ---- trajectory file encoders (jamun_traj.hip) ----------------------------------------------------------------------------------------

int jamun_pdb_models_nbytes(int64_t body_len, int64_t first_model, int64_t n_frames, int64_t* nbytes) {
  return guarded([&] {
    if (!nbytes) throw Err(JAMUN_ERR_INVALID, "null argument");
    *nbytes = checked_pdb_nbytes(body_len, first_model, n_frames);
  });
}

int jamun_encode_pdb_models(const float* xyz_dev, int64_t frame_stride, int64_t atom_stride, int32_t n_atoms, int32_t n_frames, int64_t first_model,
                            const uint8_t* body_dev, int64_t body_len, const int32_t* coord_off_dev, uint8_t* out_dev, int64_t out_capacity,
                            uint32_t* unencodable_dev, void* stream) {
  return guarded([&] {
    const FramesView in{xyz_dev, frame_stride, atom_stride, n_atoms, n_frames};
    if (!in.ptr || !body_dev || !coord_off_dev || !out_dev || !unencodable_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (in.negative() || out_capacity < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    if ((int64_t)n_atoms + 1 > 99999) throw Err(JAMUN_ERR_INVALID, "n_atoms + 1 > 99999: the serial field of the ATOM / TER records would widen");
    const int64_t need = checked_pdb_nbytes(body_len, first_model, n_frames);
    require_capacity("out_capacity", out_capacity, need, "models", "bytes");
    if (n_frames == 0) return;
    launch_encode_pdb(xyz_dev, frame_stride, atom_stride, n_atoms, n_frames, first_model, body_dev, (int)body_len, coord_off_dev, out_dev,
                      unencodable_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_encode_dcd_frames(const float* xyz_dev, int64_t frame_stride, int64_t atom_stride, int32_t n_atoms, int32_t n_frames, uint8_t* out_dev,
                            int64_t out_capacity, void* stream) {
  return guarded([&] {
    const FramesView in{xyz_dev, frame_stride, atom_stride, n_atoms, n_frames};
    if (!in.ptr || !out_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (in.negative() || out_capacity < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    if (reinterpret_cast<uintptr_t>(out_dev) & 3) throw Err(JAMUN_ERR_INVALID, "out_dev must be 4-byte aligned");
    const int64_t need = (int64_t)n_frames * 3 * (4 * (int64_t)n_atoms + 8);
    require_capacity("out_capacity", out_capacity, need, "frames", "bytes");
    if (n_frames == 0) return;
    launch_encode_dcd(xyz_dev, frame_stride, atom_stride, n_atoms, n_frames, out_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

// ---- superposition (jamun_superpose.hip) -------------------------------------------------------------------------------------------------

int jamun_superpose_frames(const float* xyz_dev, int64_t frame_stride, int64_t atom_stride, int32_t n_atoms, int32_t n_frames, const float* ref_dev,
                           float* out_dev, int64_t out_frame_stride, int64_t out_atom_stride, float* rmsd_dev, void* stream) {
  return guarded([&] {
    const FramesView in{xyz_dev, frame_stride, atom_stride, n_atoms, n_frames}, out{out_dev, out_frame_stride, out_atom_stride, n_atoms, n_frames};
    if (!in.ptr || !ref_dev || !out.ptr) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (in.negative() || out.negative()) throw Err(JAMUN_ERR_INVALID, "negative argument");
    if (n_frames == 0 || n_atoms == 0) return;  // (no frame, or frames without atoms: nothing to write, no RMSD to define)
    const bool in_place = out_dev == xyz_dev && out_frame_stride == frame_stride && out_atom_stride == atom_stride;
    if (!in_place) {
      const unsigned __int128 a0 = reinterpret_cast<uintptr_t>(xyz_dev), b0 = reinterpret_cast<uintptr_t>(out_dev);
      const unsigned __int128 a1 = a0 + 4 * in.span();
      const unsigned __int128 b1 = b0 + 4 * out.span();
      if (a0 < b1 && b0 < a1)
        throw Err(JAMUN_ERR_INVALID, "out_dev overlaps xyz_dev: the output may be the input itself with the same strides (in place), or memory apart from it");
    }
    launch_superpose_frames(xyz_dev, frame_stride, atom_stride, n_atoms, n_frames, ref_dev, out_dev, out_frame_stride, out_atom_stride, rmsd_dev,
                            (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

// ---- internal coordinates (jamun_intcoord.hip) ---------------------------------------------------------------------------------------------

int jamun_internal_coords(const float* xyz_dev, int64_t frame_stride, int64_t atom_stride, int32_t n_atoms, int32_t n_frames, const int32_t* idx_dev,
                          int32_t n_feat, int32_t cossin, float* out_dev, int64_t out_capacity, void* stream) {
  return guarded([&] {
    const FramesView in{xyz_dev, frame_stride, atom_stride, n_atoms, n_frames};
    if (in.negative() || n_feat < 0 || out_capacity < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    const int64_t need = (int64_t)n_frames * (int64_t)n_feat * (cossin ? 2 : 1);  // (< 2^63: two 31-bit counts and a factor 2)
    require_capacity("out_capacity", out_capacity, need, "features", "floats");
    if (n_frames == 0 || n_feat == 0) return;  // (nothing to write)
    if (!in.ptr || !idx_dev || !out_dev) throw Err(JAMUN_ERR_INVALID, "null argument");  // (after the empty return: an empty call may pass null)
    launch_internal_coords(xyz_dev, frame_stride, atom_stride, n_atoms, n_frames, idx_dev, n_feat, cossin != 0, out_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

// ---- histograms of angle pairs and their Jensen-Shannon divergence (jamun_hist.hip) --------------------------------------------------------

int jamun_hist2d_pairs(const float* angles_dev, int64_t row_stride, int32_t n_frames, int32_t width, const int32_t* pairs_dev, int32_t n_pairs,
                       const double* edges_dev, int32_t bins, const int32_t* cuts, int32_t n_cuts, uint32_t* counts_dev,
                       int64_t counts_capacity, uint32_t* skipped_dev, void* stream) {
  return guarded([&] {
    if (row_stride < 0 || n_frames < 0 || width < 0 || n_pairs < 0 || counts_capacity < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    check_range("bins", bins, 1, JAMUN_HIST_MAX_BINS);
    const JamunHistCuts k = parse_cuts(cuts, n_cuts, n_frames);
    check_row_stride(row_stride, width, "the width ");
    if (n_pairs > 65535) throw Err(JAMUN_ERR_INVALID, "n_pairs " + std::to_string(n_pairs) + " is above 65535");
    const int64_t need = (int64_t)n_cuts * (int64_t)n_pairs * bins * bins;  // (< 2^37)
    require_capacity("counts_capacity", counts_capacity, need, "histograms", "counters");
    if (n_pairs == 0) return;  // (nothing to write)
    if (!angles_dev || !pairs_dev || !edges_dev || !counts_dev || !skipped_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    HIPCHECK(hipMemsetAsync(counts_dev, 0, (size_t)need * sizeof(uint32_t), st));
    HIPCHECK(hipMemsetAsync(skipped_dev, 0, (size_t)n_cuts * n_pairs * sizeof(uint32_t), st));
    launch_hist2d_pairs(angles_dev, row_stride, width, pairs_dev, n_pairs, edges_dev, bins, k, counts_dev, skipped_dev, st);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_js_divergence(const uint32_t* counts_dev, int32_t n_cuts, int32_t n_pairs, int32_t bins, const uint32_t* ref_dev, int32_t n_ref_pairs,
                        double* pooled_dev, double* per_pair_dev, void* stream) {
  return guarded([&] {
    check_range("bins", bins, 1, JAMUN_HIST_MAX_BINS);
    check_range("n_cuts", n_cuts, 1, JAMUN_HIST_MAX_CUTS);
    check_range("n_pairs", n_pairs, 1, 65534);
    if (n_ref_pairs != 1 && n_ref_pairs != n_pairs)
      throw Err(JAMUN_ERR_INVALID, "n_ref_pairs " + std::to_string(n_ref_pairs) + " is neither 1 nor n_pairs = " + std::to_string(n_pairs));
    if (!counts_dev || !ref_dev || !pooled_dev || !per_pair_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    launch_js_divergence(counts_dev, n_cuts, n_pairs, bins, ref_dev, n_ref_pairs, pooled_dev, per_pair_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

// ---- chemical validity of frames (jamun_validity.hip) --------------------------------------------------------------------------------------

int jamun_validity_counts(const float* xyz_dev, int64_t frame_stride, int64_t atom_stride, int32_t n_atoms, int32_t n_frames, const float* clash_s_dev,
                          const int32_t* bonds_dev, const float* bond_lo_s_dev, const float* bond_hi_s_dev, int32_t n_bonds, uint32_t* counts_dev,
                          int64_t counts_capacity, uint32_t* bond_frames_dev, void* stream) {
  return guarded([&] {
    // (not FramesView::negative: a negative n_atoms is answered with its range below)
    if (frame_stride < 0 || atom_stride < 0 || n_frames < 0 || n_bonds < 0 || counts_capacity < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    check_range("n_atoms", n_atoms, 1, JAMUN_VALIDITY_MAX_ATOMS);
    const int64_t need = 2 * (int64_t)n_frames;
    require_capacity("counts_capacity", counts_capacity, need, "frames", "counters");
    if (n_frames == 0) return;  // (nothing to write)
    if (!xyz_dev || !counts_dev || (n_atoms > 1 && !clash_s_dev) || (n_bonds > 0 && (!bonds_dev || !bond_lo_s_dev || !bond_hi_s_dev)))
      throw Err(JAMUN_ERR_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (bond_frames_dev && n_bonds > 0) HIPCHECK(hipMemsetAsync(bond_frames_dev, 0, (size_t)n_bonds * sizeof(uint32_t), st));
    launch_validity_frames(xyz_dev, frame_stride, atom_stride, n_atoms, n_frames, clash_s_dev, bonds_dev, bond_lo_s_dev, bond_hi_s_dev, n_bonds,
                           counts_dev, bond_frames_dev, st);
    HIPCHECK(hipGetLastError());
  });
}

// ---- lagged moments, projection and autocovariance sums of feature trajectories (jamun_tica.hip) ----------------------------------------------

int jamun_lagged_moments_work(int32_t n_frames, int32_t width, int32_t lag, int64_t* n_doubles) {
  return guarded([&] {
    if (!n_doubles) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (n_frames < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    check_range("width", width, 1, JAMUN_TICA_MAX_WIDTH);
    if (n_frames == 0) {
      *n_doubles = 0;
      return;
    }
    check_tica_lag(lag, n_frames);
    *n_doubles = moments_work_doubles(n_frames, width, lag);
  });
}

int jamun_lagged_moments(const float* x_dev, int64_t row_stride, int32_t n_frames, int32_t width, int32_t lag, double* sums_dev, double* moments_dev,
                         double* work_dev, int64_t work_capacity, void* stream) {
  return guarded([&] {
    if (row_stride < 0 || n_frames < 0 || work_capacity < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    check_range("width", width, 1, JAMUN_TICA_MAX_WIDTH);
    if (n_frames == 0) return;  // (nothing to write)
    check_tica_lag(lag, n_frames);
    check_row_stride(row_stride, width, "the width ");
    require_capacity("work_capacity", work_capacity, moments_work_doubles(n_frames, width, lag), "partial sums", "doubles");
    if (!x_dev || !sums_dev || !moments_dev || !work_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    launch_lagged_moments(x_dev, row_stride, n_frames, width, lag, sums_dev, moments_dev, work_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_project_frames(const float* x_dev, int64_t row_stride, int32_t n_frames, int32_t width, const double* mean_dev, const double* v_dev, int32_t d,
                         double* out_dev, int64_t out_capacity, void* stream) {
  return guarded([&] {
    if (row_stride < 0 || n_frames < 0 || out_capacity < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    check_range("width", width, 1, JAMUN_TICA_MAX_WIDTH);
    if (d < 1 || d > width) throw Err(JAMUN_ERR_INVALID, "d " + std::to_string(d) + " is outside [1, width = " + std::to_string(width) + "]");
    check_row_stride(row_stride, width, "the width ");
    require_capacity("out_capacity", out_capacity, (int64_t)n_frames * d, "projections", "doubles");
    if (n_frames == 0) return;  // (nothing to write)
    if (!x_dev || !mean_dev || !v_dev || !out_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    launch_project_frames(x_dev, row_stride, n_frames, width, mean_dev, v_dev, d, out_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_autocov_sums_work(int32_t n_frames, int32_t max_lag, int64_t* n_doubles) {
  return guarded([&] {
    if (!n_doubles) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (n_frames < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    check_range("max_lag", max_lag, 0, JAMUN_TICA_MAX_ACF_LAG);
    *n_doubles = n_frames == 0 ? 0 : autocov_work_doubles(n_frames, max_lag);
  });
}

int jamun_autocov_sums(const double* y_dev, int64_t stride, int32_t n_frames, int32_t max_lag, double* out_dev, double* work_dev, int64_t work_capacity,
                       void* stream) {
  return guarded([&] {
    if (stride < 0 || n_frames < 0 || work_capacity < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    check_range("max_lag", max_lag, 0, JAMUN_TICA_MAX_ACF_LAG);
    if (n_frames == 0) return;  // (nothing to write)
    if (stride < 1) throw Err(JAMUN_ERR_INVALID, "stride 0: the values of y must lie apart");
    require_capacity("work_capacity", work_capacity, autocov_work_doubles(n_frames, max_lag), "partial sums", "doubles");
    if (!y_dev || !out_dev || !work_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    launch_autocov_sums(y_dev, stride, n_frames, max_lag, out_dev, work_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

// ---- nearest centres, cluster sums, transition and occupancy counts (jamun_msm.hip) ------------------------------------------------------------

int jamun_assign_centers(const double* y_dev, int64_t row_stride, int32_t n_frames, int32_t d, const double* centers_dev, int32_t k,
                         int32_t* labels_dev, double* sqdist_dev, const int32_t* prev_labels_dev, int64_t* n_changed_dev, void* stream) {
  return guarded([&] {
    if (row_stride < 0 || n_frames < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    check_centers(k, d);
    check_row_stride(row_stride, d, "d = ");
    if ((prev_labels_dev == nullptr) != (n_changed_dev == nullptr))
      throw Err(JAMUN_ERR_INVALID, "prev_labels_dev and n_changed_dev go together: one of them is null");
    if (n_frames == 0) return;  // (nothing to write)
    if (!y_dev || !centers_dev || !labels_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    launch_assign_centers(y_dev, row_stride, n_frames, d, centers_dev, k, labels_dev, sqdist_dev, prev_labels_dev, (long long*)n_changed_dev,
                          (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_cluster_sums_work(int32_t n_frames, int32_t d, int32_t k, int64_t* n_doubles) {
  return guarded([&] {
    if (!n_doubles) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (n_frames < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    check_centers(k, d);
    *n_doubles = n_frames == 0 ? 0 : cluster_work_doubles(n_frames, d, k);
  });
}

int jamun_cluster_sums(const double* y_dev, int64_t row_stride, int32_t n_frames, int32_t d, const int32_t* labels_dev, int32_t k,
                       int64_t* counts_dev, double* sums_dev, double* work_dev, int64_t work_capacity, void* stream) {
  return guarded([&] {
    if (row_stride < 0 || n_frames < 0 || work_capacity < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    check_centers(k, d);
    check_row_stride(row_stride, d, "d = ");
    if (n_frames == 0) return;  // (nothing to write)
    require_capacity("work_capacity", work_capacity, cluster_work_doubles(n_frames, d, k), "partial sums", "doubles");
    if (!y_dev || !labels_dev || !counts_dev || !sums_dev || !work_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    launch_cluster_sums(y_dev, row_stride, n_frames, d, labels_dev, k, (long long*)counts_dev, sums_dev, work_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_transition_counts(const int32_t* labels_dev, int32_t n_frames, int32_t lag, const int32_t* map_dev, int32_t n_in, int32_t n_states,
                            int64_t* counts_dev, void* stream) {
  return guarded([&] {
    if (n_frames < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    const int32_t n_labels = check_states(n_states, map_dev, n_in);
    if (lag < 1) throw Err(JAMUN_ERR_INVALID, "lag " + std::to_string(lag) + " is below 1");
    if (lag >= n_frames) return;  // (no frames, or no pair that far apart: nothing to count)
    if (!labels_dev || !counts_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    launch_transition_counts(labels_dev, n_frames, lag, map_dev, n_labels, n_states, (long long*)counts_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_label_counts(const int32_t* labels_dev, int32_t n_frames, const int32_t* map_dev, int32_t n_in, int32_t n_states,
                       const int32_t* bounds_dev, int32_t n_seg, int64_t* counts_dev, void* stream) {
  return guarded([&] {
    if (n_frames < 0) throw Err(JAMUN_ERR_INVALID, "negative argument");
    const int32_t n_labels = check_states(n_states, map_dev, n_in);
    check_range("n_seg", n_seg, 1, JAMUN_MSM_MAX_SEGMENTS);
    if (n_frames == 0) return;  // (nothing to count)
    if (!labels_dev || !bounds_dev || !counts_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    launch_label_counts(labels_dev, n_frames, map_dev, n_labels, n_states, bounds_dev, n_seg, (long long*)counts_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

// ---- sliced Wasserstein distance: projection, segment sort, merge, quantile integral (jamun_swd.hip) -----------------------------------------

int jamun_swd_project(const float* x_dev, int64_t row_stride, int32_t n_frames, int32_t width, const float* proj_dev, int32_t n_proj, float* out_dev,
                      int64_t out_capacity, void* stream) {
  return guarded([&] {
    check_range("n_frames", n_frames, 1, INT32_MAX);
    check_range("width", width, 1, JAMUN_SWD_MAX_WIDTH);
    check_range("n_proj", n_proj, 1, JAMUN_SWD_MAX_PROJ);
    check_row_stride(row_stride, width, "the width ");
    require_capacity("out_capacity", out_capacity, (int64_t)n_frames * n_proj, "keys", "floats");
    if (!x_dev || !proj_dev || !out_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    launch_swd_project(x_dev, row_stride, n_frames, width, proj_dev, n_proj, out_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_swd_sort_work(int32_t n_frames, int32_t n_proj, const int32_t* cuts, int32_t n_cuts, int64_t* n_floats) {
  return guarded([&] {
    if (!n_floats) throw Err(JAMUN_ERR_INVALID, "null argument");
    *n_floats = swd_sort_work_floats(n_frames, n_proj, swd_cuts(n_frames, n_proj, cuts, n_cuts));
  });
}

int jamun_swd_sort_segments(const float* keys_dev, int32_t n_frames, int32_t n_proj, const int32_t* cuts, int32_t n_cuts, float* out_dev,
                            int64_t out_capacity, float* work_dev, int64_t work_capacity, void* stream) {
  return guarded([&] {
    const JamunHistCuts k = swd_cuts(n_frames, n_proj, cuts, n_cuts);
    require_capacity("out_capacity", out_capacity, (int64_t)n_frames * n_proj, "keys", "floats");
    const int64_t need = swd_sort_work_floats(n_frames, n_proj, k);
    require_capacity("work_capacity", work_capacity, need, "merge passes", "floats");
    if (!keys_dev || !out_dev || (need > 0 && !work_dev)) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (need > 0 && work_dev < out_dev + (int64_t)n_frames * n_proj && out_dev < work_dev + need)
      throw Err(JAMUN_ERR_INVALID, "work_dev overlaps out_dev");
    HIPCHECK(launch_swd_sort_segments(keys_dev, n_frames, n_proj, k, out_dev, work_dev, (hipStream_t)stream));
    HIPCHECK(hipGetLastError());
  });
}

int jamun_swd_merge(const float* a_dev, int64_t a_stride, int32_t n, const float* b_dev, int64_t b_stride, int32_t m, int32_t n_proj, float* out_dev,
                    int64_t out_capacity, void* stream) {
  return guarded([&] {
    swd_columns(a_stride, n, b_stride, m, n_proj);
    if ((int64_t)n + m > INT32_MAX) throw Err(JAMUN_ERR_INVALID, "n + m = " + std::to_string((int64_t)n + m) + " does not fit 31 bits");
    require_capacity("out_capacity", out_capacity, ((int64_t)n + m) * n_proj, "merged columns", "floats");
    if (!a_dev || !b_dev || !out_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    launch_swd_merge(a_dev, a_stride, n, b_dev, b_stride, m, n_proj, out_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_swd_w2sq_work(int32_t n, int32_t m, int32_t n_proj, int64_t* n_doubles) {
  return guarded([&] {
    if (!n_doubles) throw Err(JAMUN_ERR_INVALID, "null argument");
    swd_columns(n, n, m, m, n_proj);
    *n_doubles = swd_w2sq_work_doubles(n, m, n_proj);
  });
}

int jamun_swd_w2sq(const float* u_dev, int64_t u_stride, int32_t n, const float* v_dev, int64_t v_stride, int32_t m, int32_t n_proj, double* out_dev,
                   double* work_dev, int64_t work_capacity, void* stream) {
  return guarded([&] {
    swd_columns(u_stride, n, v_stride, m, n_proj);
    require_capacity("work_capacity", work_capacity, swd_w2sq_work_doubles(n, m, n_proj), "partial sums", "doubles");
    if (!u_dev || !v_dev || !out_dev || !work_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    launch_swd_w2sq(u_dev, u_stride, n, v_dev, v_stride, m, n_proj, out_dev, work_dev, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

}  // extern "C"
