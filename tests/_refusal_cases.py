"""The refusals of the frame-analysis bindings as a named table of bad calls, shared by tests/golden/make_frames_refusals.py (which records
what each case answers into tests/golden/frames_refusals.json) and tests/test_frames_refusals_host.py (which holds the tree to the record).
No case needs a GPU.

Part A, `C_CASES`: the C entries of csrc/jamun_frames.cpp through ctypes.  Every device pointer an entry requires is null, and every entry
refuses a required null pointer before it launches anything, so no case can reach a kernel on any machine, even if the check it aims at were
lost: the null-argument refusal, last in line, would still end the call.  Host pointers (``cuts``, the out-parameter of a ``*_work`` query)
are real.  Two cases (`HOST` below) hand one OPTIONAL device argument a host address, since "go together" and "a map has at least one entry"
cannot be asked for otherwise; the required pointers of those calls are null like everywhere else.  What an entry refuses only AFTER its
null check stays with the GPU tests: the ``work_dev`` / ``out_dev`` overlap of ``jamun_swd_sort_segments`` (tests/test_gpu_swd.py) and the
``out_dev`` overlap of ``jamun_superpose_frames`` (tests/test_gpu_superpose.py) need pointers that are not null.

Part B, `PY_CASES`: the Python entry points, addressed through ``jamun_amd.native``, with CPU tensors, host arrays and bad scalars: every
case raises before a GPU is needed.  A wrong ``out=`` is met only behind the check that the input is on a GPU, so it is asked of `_result`,
which every entry hands its ``out=`` to, directly (and a wrong device table of `_table` likewise).  `transition_counts` and `label_counts`
check their labels, which must be on a GPU, before anything else: their ``n_states`` and ``state_map`` rules are asked of `_state_map`, which
both hand them to, directly; the ``lag`` of `transition_counts` and the ``bounds`` and the segment count of `label_counts` cannot be reached
without a GPU and are pinned in tests/test_gpu_msm.py.  What `_state_map` ACCEPTS of a host table (a scalar, floats) is no refusal and is
pinned in tests/test_frames_refusals_host.py.
"""
import ctypes as C

import numpy as np
import torch

OUT = "out"    # an int64 the entry writes to (the out-parameter of a *_work query)
HOST = "host"  # the address of 64 bytes of host memory, for an optional device argument (see above)
BIG = 1 << 40  # a capacity no case exceeds
I31 = 0x7FFFFFFF

# entry -> its arguments in order, as one call that every check but the null-argument one lets through
C_ENTRIES = {
    "jamun_pdb_models_nbytes": dict(body_len=100, first_model=1, n_frames=3, nbytes=OUT),
    "jamun_encode_pdb_models": dict(xyz_dev=None, frame_stride=30, atom_stride=3, n_atoms=10, n_frames=2, first_model=1, body_dev=None, body_len=100,
                                    coord_off_dev=None, out_dev=None, out_capacity=BIG, unencodable_dev=None, stream=None),
    "jamun_encode_dcd_frames": dict(xyz_dev=None, frame_stride=30, atom_stride=3, n_atoms=10, n_frames=2, out_dev=None, out_capacity=BIG, stream=None),
    "jamun_superpose_frames": dict(xyz_dev=None, frame_stride=30, atom_stride=3, n_atoms=10, n_frames=2, ref_dev=None, out_dev=None,
                                   out_frame_stride=30, out_atom_stride=3, rmsd_dev=None, stream=None),
    "jamun_internal_coords": dict(xyz_dev=None, frame_stride=30, atom_stride=3, n_atoms=10, n_frames=2, idx_dev=None, n_feat=4, cossin=1, out_dev=None,
                                  out_capacity=16, stream=None),
    "jamun_hist2d_pairs": dict(angles_dev=None, row_stride=8, n_frames=100, width=8, pairs_dev=None, n_pairs=2, edges_dev=None, bins=4, cuts=[50, 100],
                               n_cuts=2, counts_dev=None, counts_capacity=64, skipped_dev=None, stream=None),
    "jamun_js_divergence": dict(counts_dev=None, n_cuts=2, n_pairs=3, bins=4, ref_dev=None, n_ref_pairs=3, pooled_dev=None, per_pair_dev=None, stream=None),
    "jamun_validity_counts": dict(xyz_dev=None, frame_stride=30, atom_stride=3, n_atoms=10, n_frames=2, clash_s_dev=None, bonds_dev=None,
                                  bond_lo_s_dev=None, bond_hi_s_dev=None, n_bonds=3, counts_dev=None, counts_capacity=4, bond_frames_dev=None, stream=None),
    "jamun_lagged_moments_work": dict(n_frames=100, width=8, lag=5, n_doubles=OUT),
    "jamun_lagged_moments": dict(x_dev=None, row_stride=8, n_frames=100, width=8, lag=5, sums_dev=None, moments_dev=None, work_dev=None,
                                 work_capacity=BIG, stream=None),
    "jamun_project_frames": dict(x_dev=None, row_stride=8, n_frames=100, width=8, mean_dev=None, v_dev=None, d=2, out_dev=None, out_capacity=200,
                                 stream=None),
    "jamun_autocov_sums_work": dict(n_frames=100, max_lag=10, n_doubles=OUT),
    "jamun_autocov_sums": dict(y_dev=None, stride=2, n_frames=100, max_lag=10, out_dev=None, work_dev=None, work_capacity=BIG, stream=None),
    "jamun_assign_centers": dict(y_dev=None, row_stride=2, n_frames=100, d=2, centers_dev=None, k=5, labels_dev=None, sqdist_dev=None,
                                 prev_labels_dev=None, n_changed_dev=None, stream=None),
    "jamun_cluster_sums_work": dict(n_frames=100, d=2, k=5, n_doubles=OUT),
    "jamun_cluster_sums": dict(y_dev=None, row_stride=2, n_frames=100, d=2, labels_dev=None, k=5, counts_dev=None, sums_dev=None, work_dev=None,
                               work_capacity=BIG, stream=None),
    "jamun_transition_counts": dict(labels_dev=None, n_frames=100, lag=5, map_dev=None, n_in=0, n_states=4, counts_dev=None, stream=None),
    "jamun_label_counts": dict(labels_dev=None, n_frames=100, map_dev=None, n_in=0, n_states=4, bounds_dev=None, n_seg=2, counts_dev=None, stream=None),
    "jamun_swd_project": dict(x_dev=None, row_stride=8, n_frames=100, width=8, proj_dev=None, n_proj=4, out_dev=None, out_capacity=400, stream=None),
    "jamun_swd_sort_work": dict(n_frames=100, n_proj=4, cuts=[50, 100], n_cuts=2, n_floats=OUT),
    "jamun_swd_sort_segments": dict(keys_dev=None, n_frames=100, n_proj=4, cuts=[50, 100], n_cuts=2, out_dev=None, out_capacity=400, work_dev=None,
                                    work_capacity=BIG, stream=None),
    "jamun_swd_merge": dict(a_dev=None, a_stride=60, n=60, b_dev=None, b_stride=40, m=40, n_proj=4, out_dev=None, out_capacity=400, stream=None),
    "jamun_swd_w2sq_work": dict(n=60, m=40, n_proj=4, n_doubles=OUT),
    "jamun_swd_w2sq": dict(u_dev=None, u_stride=60, n=60, v_dev=None, v_stride=40, m=40, n_proj=4, out_dev=None, work_dev=None, work_capacity=BIG,
                           stream=None),
}

_BAD_CUTS = dict(bad_n_cuts=dict(n_cuts=65), zero_cuts=dict(n_cuts=0), null_cuts=dict(cuts=None), cut_below_1=dict(cuts=[0, 100]),
                 cut_above_frames=dict(cuts=[50, 101]), cuts_not_ascending=dict(cuts=[50, 50]), n_cuts_then_null_cuts=dict(n_cuts=65, cuts=None),
                 null_cuts_then_ascent=dict(cuts=None, n_frames=10))

# entry -> {case: the arguments that differ from C_ENTRIES}; "a_then_b" has both faults and pins that a is the one reported
_C = {
    "jamun_pdb_models_nbytes": dict(null=dict(nbytes=None), null_then_negative=dict(nbytes=None, body_len=-1), negative=dict(n_frames=-1),
                                    body_31_bits=dict(body_len=1 << 31), model_number=dict(first_model=10**15 + 1),
                                    negative_then_model_number=dict(body_len=-1, n_frames=10**15 + 1),
                                    body_then_model_number=dict(body_len=1 << 31, first_model=10**15 + 1)),
    "jamun_encode_pdb_models": dict(null=dict(), null_then_negative=dict(frame_stride=-1), null_then_atoms=dict(n_atoms=99999),
                                    null_then_capacity=dict(out_capacity=0)),
    "jamun_encode_dcd_frames": dict(null=dict(), null_then_negative=dict(n_frames=-1), null_then_capacity=dict(out_capacity=0)),
    "jamun_superpose_frames": dict(null=dict(), null_then_negative=dict(out_atom_stride=-1)),
    "jamun_internal_coords": dict(null=dict(), negative_stride=dict(atom_stride=-1), negative_features=dict(n_feat=-1), negative_capacity=dict(out_capacity=-1),
                                  capacity=dict(out_capacity=15), capacity_plain=dict(cossin=0, out_capacity=7),
                                  negative_then_capacity=dict(n_frames=-1, out_capacity=0), capacity_then_null=dict(out_capacity=0)),
    "jamun_hist2d_pairs": dict(null=dict(), negative=dict(width=-1), negative_then_bins=dict(n_pairs=-1, bins=0), bins_low=dict(bins=0), bins_high=dict(bins=129),
                               bins_then_n_cuts=dict(bins=129, n_cuts=0), **_BAD_CUTS, cuts_then_stride=dict(cuts=[50, 40], row_stride=7),
                               stride=dict(row_stride=7), stride_then_pairs=dict(row_stride=7, n_pairs=65536), pairs=dict(n_pairs=65536, counts_capacity=BIG),
                               pairs_then_capacity=dict(n_pairs=65536), capacity=dict(counts_capacity=63), capacity_then_null=dict(counts_capacity=0)),
    "jamun_js_divergence": dict(null=dict(), bins_low=dict(bins=0), bins_high=dict(bins=129), bins_then_n_cuts=dict(bins=0, n_cuts=65), n_cuts=dict(n_cuts=0),
                                n_cuts_then_pairs=dict(n_cuts=65, n_pairs=0), pairs_low=dict(n_pairs=0, n_ref_pairs=1), pairs_high=dict(n_pairs=65535),
                                pairs_then_ref=dict(n_pairs=0, n_ref_pairs=2), ref_pairs=dict(n_ref_pairs=2), one_ref_pair_null=dict(n_ref_pairs=1)),
    "jamun_validity_counts": dict(null=dict(), negative=dict(n_bonds=-1), negative_then_atoms=dict(frame_stride=-1, n_atoms=0), atoms_low=dict(n_atoms=0),
                                  atoms_negative=dict(n_atoms=-1), atoms_high=dict(n_atoms=257), atoms_then_capacity=dict(n_atoms=257, counts_capacity=0),
                                  capacity=dict(counts_capacity=3), one_atom_no_bonds_null=dict(n_atoms=1, n_bonds=0)),
    "jamun_lagged_moments_work": dict(null=dict(n_doubles=None), null_then_negative=dict(n_doubles=None, n_frames=-1), negative=dict(n_frames=-1),
                                      negative_then_width=dict(n_frames=-1, width=0), width_low=dict(width=0), width_high=dict(width=129),
                                      width_then_lag=dict(width=129, lag=0), lag_low=dict(lag=0), lag_high=dict(lag=100)),
    "jamun_lagged_moments": dict(null=dict(), negative=dict(work_capacity=-1), negative_then_width=dict(row_stride=-1, width=129), width=dict(width=0),
                                 width_then_lag=dict(width=0, lag=0), lag_low=dict(lag=0), lag_high=dict(lag=100), lag_then_stride=dict(lag=100, row_stride=7),
                                 stride=dict(row_stride=7), stride_then_capacity=dict(row_stride=7, work_capacity=0), capacity=dict(work_capacity=0)),
    "jamun_project_frames": dict(null=dict(), negative=dict(n_frames=-1), negative_then_width=dict(out_capacity=-1, width=0), width=dict(width=129),
                                 width_then_d=dict(width=0, d=0), d_low=dict(d=0), d_high=dict(d=9), d_then_stride=dict(d=9, row_stride=7), stride=dict(row_stride=7),
                                 stride_then_capacity=dict(row_stride=7, out_capacity=0), capacity=dict(out_capacity=199)),
    "jamun_autocov_sums_work": dict(null=dict(n_doubles=None), null_then_lag=dict(n_doubles=None, max_lag=-1), negative=dict(n_frames=-1),
                                    negative_then_lag=dict(n_frames=-1, max_lag=4097), lag_low=dict(max_lag=-1), lag_high=dict(max_lag=4097)),
    "jamun_autocov_sums": dict(null=dict(), negative=dict(stride=-1), negative_then_lag=dict(work_capacity=-1, max_lag=-1), lag_low=dict(max_lag=-1),
                               lag_high=dict(max_lag=4097), lag_then_stride=dict(max_lag=4097, stride=0), stride=dict(stride=0),
                               stride_then_capacity=dict(stride=0, work_capacity=0), capacity=dict(work_capacity=0)),
    "jamun_assign_centers": dict(null=dict(), negative=dict(n_frames=-1), negative_then_k=dict(row_stride=-1, k=0), k_low=dict(k=0), k_high=dict(k=1025),
                                 k_then_d=dict(k=0, d=0), d_low=dict(d=0), d_high=dict(d=129, row_stride=129), kd=dict(k=1024, d=17, row_stride=17),
                                 kd_then_stride=dict(k=1024, d=17), stride=dict(row_stride=1), stride_then_pair=dict(row_stride=1, prev_labels_dev=HOST),
                                 prev_without_changed=dict(prev_labels_dev=HOST), changed_without_prev=dict(n_changed_dev=HOST)),
    "jamun_cluster_sums_work": dict(null=dict(n_doubles=None), null_then_negative=dict(n_doubles=None, n_frames=-1), negative=dict(n_frames=-1),
                                    negative_then_k=dict(n_frames=-1, k=0), k=dict(k=1025), d=dict(d=129), kd=dict(k=1024, d=17)),
    "jamun_cluster_sums": dict(null=dict(), negative=dict(work_capacity=-1), negative_then_k=dict(n_frames=-1, k=0), k=dict(k=0), d=dict(d=0),
                               kd=dict(k=1024, d=17, row_stride=17), k_then_stride=dict(k=1025, row_stride=1), stride=dict(row_stride=1),
                               stride_then_capacity=dict(row_stride=1, work_capacity=0), capacity=dict(work_capacity=0)),
    "jamun_transition_counts": dict(null=dict(), negative=dict(n_frames=-1), negative_then_states=dict(n_frames=-1, n_states=0), states_low=dict(n_states=0),
                                    states_high=dict(n_states=1025), states_then_map=dict(n_states=0, map_dev=HOST), empty_map=dict(map_dev=HOST),
                                    map_then_lag=dict(map_dev=HOST, lag=0), lag=dict(lag=0), lag_then_null=dict(lag=-1)),
    "jamun_label_counts": dict(null=dict(), negative=dict(n_frames=-1), negative_then_states=dict(n_frames=-1, n_states=1025), states=dict(n_states=0),
                               empty_map=dict(map_dev=HOST), states_then_segments=dict(n_states=0, n_seg=0), segments_low=dict(n_seg=0),
                               segments_high=dict(n_seg=4097)),
    "jamun_swd_project": dict(null=dict(), frames=dict(n_frames=0), frames_then_width=dict(n_frames=-1, width=0), width_low=dict(width=0),
                              width_high=dict(width=129, row_stride=129), width_then_proj=dict(width=0, n_proj=0), proj_low=dict(n_proj=0),
                              proj_high=dict(n_proj=65, out_capacity=BIG), proj_then_stride=dict(n_proj=65, row_stride=7), stride=dict(row_stride=7),
                              negative_stride=dict(row_stride=-1), stride_then_capacity=dict(row_stride=7, out_capacity=0), capacity=dict(out_capacity=399),
                              negative_capacity=dict(out_capacity=-1)),
    "jamun_swd_sort_work": dict(null=dict(n_floats=None), null_then_frames=dict(n_floats=None, n_frames=0), frames=dict(n_frames=0),
                                frames_then_proj=dict(n_frames=0, n_proj=0), proj_low=dict(n_proj=0), proj_high=dict(n_proj=65),
                                proj_then_n_cuts=dict(n_proj=65, n_cuts=0), **_BAD_CUTS),
    "jamun_swd_sort_segments": dict(null=dict(), frames=dict(n_frames=0), frames_then_proj=dict(n_frames=0, n_proj=65), proj=dict(n_proj=0),
                                    proj_then_n_cuts=dict(n_proj=0, n_cuts=65), **_BAD_CUTS, cuts_then_capacity=dict(cuts=[100, 50], out_capacity=0),
                                    out_capacity=dict(out_capacity=399), out_then_work_capacity=dict(out_capacity=399, work_capacity=0),
                                    work_capacity=dict(n_frames=10000, cuts=[10000], n_cuts=1, out_capacity=BIG, work_capacity=0)),
    "jamun_swd_merge": dict(null=dict(), n=dict(n=0), n_then_m=dict(n=0, m=0), m=dict(m=-1), m_then_proj=dict(m=0, n_proj=0), proj_low=dict(n_proj=0),
                            proj_high=dict(n_proj=65), proj_then_strides=dict(n_proj=65, a_stride=59), a_stride=dict(a_stride=59), b_stride=dict(b_stride=39),
                            strides_then_sum=dict(n=I31, m=I31, a_stride=0, b_stride=I31), sum=dict(n=I31, m=1, a_stride=I31, b_stride=1),
                            sum_then_capacity=dict(n=I31, m=I31, a_stride=I31, b_stride=I31, out_capacity=0), capacity=dict(out_capacity=399)),
    "jamun_swd_w2sq_work": dict(null=dict(n_doubles=None), null_then_n=dict(n_doubles=None, n=0), n=dict(n=0), n_then_m=dict(n=0, m=0), m=dict(m=0),
                                m_then_proj=dict(m=0, n_proj=65), proj=dict(n_proj=65)),
    "jamun_swd_w2sq": dict(null=dict(), n=dict(n=0), n_then_proj=dict(n=0, n_proj=0), m=dict(m=0), proj=dict(n_proj=0), proj_then_strides=dict(n_proj=0, u_stride=1),
                           u_stride=dict(u_stride=59), v_stride=dict(v_stride=-1), strides_then_capacity=dict(v_stride=39, work_capacity=0),
                           capacity=dict(work_capacity=0), negative_capacity=dict(work_capacity=-1)),
}

C_CASES = {f"{entry}/{case}": (entry, list({**C_ENTRIES[entry], **changes}.values())) for entry, cases in _C.items() for case, changes in cases.items()}


def c_answer(lib, entry: str, args: list) -> dict:
    """One call of a C entry -> ``{"code", "text"}``: an int stands for itself, None is null, `OUT` an int64 to write to, `HOST` a host
    address, a list an int32 host array."""
    host, value, keep, call = C.create_string_buffer(64), C.c_int64(-1), [], []
    for a in args:
        if a is None or isinstance(a, int):
            call.append(a)
        elif a == OUT:
            call.append(C.byref(value))
        elif a == HOST:
            call.append(C.addressof(host))
        else:
            keep.append((C.c_int32 * len(a))(*a))
            call.append(C.cast(keep[-1], C.c_void_p))
    code = getattr(lib, entry)(*call)
    return {"code": code, "text": lib.jamun_last_error().decode() if code else ""}


def _z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def _tables(n=3, **changes):
    t = dict(clash_s=np.ones(n * (n - 1) // 2, np.float32), bonds=np.array([[0, 1], [1, 2]]), bond_lo_s=np.ones(2, np.float32), bond_hi_s=np.ones(2, np.float32))
    return {**t, **changes}


_IDX = [[0, 1, -1, -1], [0, 1, 2, -1]]
_LABELS = lambda: _z(10, dtype=torch.int32)  # noqa: E731

# case -> (function of jamun_amd.native, a callable that makes (args, kwargs)): made at call time, so that importing this table makes nothing
PY_CASES = {
    "pdb_models_nbytes/negative": ("pdb_models_nbytes", lambda: ((100, -1, 3), {})),
    "pdb_models_nbytes/body_then_model_number": ("pdb_models_nbytes", lambda: ((1 << 31, 10**15 + 1, 3), {})),
    "encode_pdb_models/cpu": ("encode_pdb_models", lambda: ((_z(2, 3, 3), 1, _z(8, dtype=torch.uint8), _z(3, dtype=torch.int32), _z(64, dtype=torch.uint8), _z(1, dtype=torch.int32)), {})),
    "encode_pdb_models/ndim": ("encode_pdb_models", lambda: ((_z(2, 9), 1, _z(8, dtype=torch.uint8), _z(3, dtype=torch.int32), _z(64, dtype=torch.uint8), _z(1, dtype=torch.int32)), {})),
    "encode_dcd_frames/cpu": ("encode_dcd_frames", lambda: ((_z(2, 3, 3), _z(64, dtype=torch.uint8)), {})),
    "encode_dcd_frames/float64": ("encode_dcd_frames", lambda: ((_z(2, 3, 3, dtype=torch.float64), _z(64, dtype=torch.uint8)), {})),
    "superpose_frames/cpu": ("superpose_frames", lambda: ((_z(2, 3, 3), _z(3, 3)), {})),
    "superpose_frames/last_axis": ("superpose_frames", lambda: ((_z(2, 3, 4), _z(3, 3)), {})),
    "superpose_frames/frames_then_ref": ("superpose_frames", lambda: ((_z(2, 3, 3), _z(4, 3)), {})),
    "check_index_table/float": ("check_index_table", lambda: ((np.zeros((2, 4)), 5), {})),
    "check_index_table/float_tensor": ("check_index_table", lambda: ((_z(2, 4), 5), {})),
    "check_index_table/shape": ("check_index_table", lambda: ((np.zeros((2, 3), np.int64), 5), {})),
    "check_index_table/dtype_then_shape": ("check_index_table", lambda: ((np.zeros((2, 3)), 5), {})),
    "check_index_table/one_atom": ("check_index_table", lambda: (([[0, 1, -1, -1], [3, -1, -1, -1]], 5), {})),
    "check_index_table/out_of_range": ("check_index_table", lambda: (([[0, 5, -1, -1]], 5), {})),
    "check_index_table/gap": ("check_index_table", lambda: (([[0, 1, -1, 2]], 5), {})),
    "check_index_table/minus_two": ("check_index_table", lambda: (([[0, 1, -2, -1]], 5), {})),
    "internal_coords/ndim": ("internal_coords", lambda: ((_z(2, 9), _IDX), {})),
    "internal_coords/not_a_tensor": ("internal_coords", lambda: ((np.zeros((2, 3, 3), np.float32), _IDX), {})),
    "internal_coords/ndim_then_table": ("internal_coords", lambda: ((_z(2, 9), [[0, 9, -1, -1]]), {})),
    "internal_coords/table": ("internal_coords", lambda: ((_z(2, 3, 3), [[0, 3, -1, -1]]), {})),
    "internal_coords/table_then_cpu": ("internal_coords", lambda: ((_z(2, 3, 3, dtype=torch.float64), np.zeros((2, 4))), {})),
    "internal_coords/cpu": ("internal_coords", lambda: ((_z(2, 3, 3), _IDX), {"cossin": True})),
    "internal_coords/float64": ("internal_coords", lambda: ((_z(2, 3, 3, dtype=torch.float64), _IDX), {})),
    "check_cuts/float": ("check_cuts", lambda: (([1.0, 2.0], 10), {})),
    "check_cuts/empty": ("check_cuts", lambda: ((np.zeros(0, np.int64), 10), {})),
    "check_cuts/too_many": ("check_cuts", lambda: ((np.arange(1, 66), 100), {})),
    "check_cuts/two_dims": ("check_cuts", lambda: (([[1, 2]], 10), {})),
    "check_cuts/zero": ("check_cuts", lambda: (([0, 5], 10), {})),
    "check_cuts/above_frames": ("check_cuts", lambda: ((torch.tensor([5, 11]), 10), {})),
    "check_cuts/not_ascending": ("check_cuts", lambda: (([5, 5, 10], 10), {})),
    "check_hist_args/pairs_float": ("check_hist_args", lambda: ((10, 4, [[0.0, 1.0]], 8, [10]), {})),
    "check_hist_args/pairs_shape": ("check_hist_args", lambda: ((10, 4, [[0, 1, 2]], 8, [10]), {})),
    "check_hist_args/pairs_column": ("check_hist_args", lambda: ((10, 4, [[0, 1], [2, 4]], 8, [10]), {})),
    "check_hist_args/pairs_then_bins": ("check_hist_args", lambda: ((10, 4, [[0, -1]], 0, [10]), {})),
    "check_hist_args/bins_zero": ("check_hist_args", lambda: ((10, 4, [[0, 1]], 0, [10]), {})),
    "check_hist_args/bins_high": ("check_hist_args", lambda: ((10, 4, None, 129, [10]), {})),
    "check_hist_args/bins_bool": ("check_hist_args", lambda: ((10, 4, [[0, 1]], True, [10]), {})),
    "check_hist_args/bins_float": ("check_hist_args", lambda: ((10, 4, [[0, 1]], 8.0, [10]), {})),
    "check_hist_args/bins_then_cuts": ("check_hist_args", lambda: ((10, 4, [[0, 1]], "8", [11]), {})),
    "check_hist_args/cuts": ("check_hist_args", lambda: ((10, 4, [[0, 1]], 8, [11]), {})),
    "hist2d_pairs/ndim": ("hist2d_pairs", lambda: ((_z(10), [[0, 1]], 8, [10]), {})),
    "hist2d_pairs/ndim_then_bins": ("hist2d_pairs", lambda: ((_z(10, 2, 2), [[0, 1]], 0, [10]), {})),
    "hist2d_pairs/pairs": ("hist2d_pairs", lambda: ((_z(10, 4), [[0, 4]], 8, [10]), {})),
    "hist2d_pairs/bins": ("hist2d_pairs", lambda: ((_z(10, 4), [[0, 1]], 1.5, [10]), {})),
    "hist2d_pairs/cuts": ("hist2d_pairs", lambda: ((_z(10, 4), [[0, 1]], 8, [10, 5]), {})),
    "hist2d_pairs/cuts_then_cpu": ("hist2d_pairs", lambda: ((_z(10, 4, dtype=torch.float64), [[0, 1]], 8, []), {})),
    "hist2d_pairs/cpu": ("hist2d_pairs", lambda: ((_z(10, 4), [[0, 1]], 8, [10]), {})),
    "hist2d_pairs/cpu_strided": ("hist2d_pairs", lambda: ((_z(10, 8)[:, ::2], [[0, 1]], 8, [5, 10]), {})),
    "js_divergence/dtype": ("js_divergence", lambda: ((_z(2, 3, 4, 4), _z(4, 4, dtype=torch.int32)), {})),
    "js_divergence/not_square": ("js_divergence", lambda: ((_z(2, 3, 4, 5, dtype=torch.int32), _z(4, 4, dtype=torch.int32)), {})),
    "js_divergence/counts_then_ref": ("js_divergence", lambda: ((_z(3, 4, 4, dtype=torch.int32), _z(4, 4)), {})),
    "js_divergence/ref_shape": ("js_divergence", lambda: ((_z(2, 3, 4, 4, dtype=torch.int32), _z(2, 4, 4, dtype=torch.int32)), {})),
    "js_divergence/ref_dtype": ("js_divergence", lambda: ((_z(2, 3, 4, 4, dtype=torch.int32), _z(4, 4)), {})),
    "js_divergence/bins": ("js_divergence", lambda: ((_z(1, 1, 129, 129, dtype=torch.int32), _z(129, 129, dtype=torch.int32)), {})),
    "js_divergence/no_pairs": ("js_divergence", lambda: ((_z(2, 0, 4, 4, dtype=torch.int32), _z(4, 4, dtype=torch.int32)), {})),
    "js_divergence/cuts": ("js_divergence", lambda: ((_z(65, 1, 2, 2, dtype=torch.int32), _z(2, 2, dtype=torch.int32)), {})),
    "js_divergence/cpu": ("js_divergence", lambda: ((_z(2, 3, 4, 4, dtype=torch.int32), _z(3, 4, 4, dtype=torch.int32)), {})),
    "check_validity_tables/clash_dtype": ("check_validity_tables", lambda: ((_tables(clash_s=np.ones(3)), 3), {})),
    "check_validity_tables/bonds_dtype": ("check_validity_tables", lambda: ((_tables(bonds=np.ones((2, 2), np.float32)), 3), {})),
    "check_validity_tables/dtype_then_shape": ("check_validity_tables", lambda: ((_tables(clash_s=np.ones(4, np.float32), bond_lo_s=np.ones(2)), 3), {})),
    "check_validity_tables/clash_shape": ("check_validity_tables", lambda: ((_tables(clash_s=np.ones(4, np.float32)), 3), {})),
    "check_validity_tables/clash_then_bonds": ("check_validity_tables", lambda: ((_tables(4, bonds=np.array([[0, 0]])), 3), {})),
    "check_validity_tables/bonds_shape": ("check_validity_tables", lambda: ((_tables(bonds=np.array([[0, 1, 2]])), 3), {})),
    "check_validity_tables/bond_out_of_range": ("check_validity_tables", lambda: ((_tables(bonds=np.array([[0, 1], [1, 3]])), 3), {})),
    "check_validity_tables/bond_with_itself": ("check_validity_tables", lambda: ((_tables(bonds=torch.tensor([[1, 1], [1, 2]])), 3), {})),
    "check_validity_tables/bound_shape": ("check_validity_tables", lambda: ((_tables(bond_hi_s=np.ones(3, np.float32)), 3), {})),
    "upload_validity_tables/tables": ("upload_validity_tables", lambda: ((_tables(bond_lo_s=np.ones(1, np.float32)), 3, "cpu"), {})),
    "validity_counts/ndim": ("validity_counts", lambda: ((_z(2, 9), _tables()), {})),
    "validity_counts/ndim_then_atoms": ("validity_counts", lambda: ((_z(2, 0), _tables()), {})),
    "validity_counts/no_atoms": ("validity_counts", lambda: ((_z(2, 0, 3), _tables()), {})),
    "validity_counts/too_many_atoms": ("validity_counts", lambda: ((_z(2, 257, 3), _tables()), {})),
    "validity_counts/atoms_then_tables": ("validity_counts", lambda: ((_z(2, 257, 3), _tables(clash_s=np.ones(3))), {})),
    "validity_counts/tables": ("validity_counts", lambda: ((_z(2, 3, 3), _tables(bonds=np.array([[0, 3]]))), {})),
    "validity_counts/tables_then_cpu": ("validity_counts", lambda: ((_z(2, 3, 3, dtype=torch.float64), _tables(4)), {})),
    "validity_counts/cpu": ("validity_counts", lambda: ((_z(2, 3, 3), _tables()), {})),
    "check_feature_rows/not_a_tensor": ("check_feature_rows", lambda: ((np.zeros((5, 4), np.float32),), {})),
    "check_feature_rows/ndim": ("check_feature_rows", lambda: ((_z(5),), {})),
    "check_feature_rows/no_columns": ("check_feature_rows", lambda: ((_z(5, 0),), {})),
    "check_feature_rows/too_wide": ("check_feature_rows", lambda: ((_z(5, 129),), {})),
    "lagged_moments/ndim_then_lag": ("lagged_moments", lambda: ((_z(5, 4, 1), 0), {})),
    "lagged_moments/width_then_lag": ("lagged_moments", lambda: ((_z(5, 129), 5), {})),
    "lagged_moments/lag_float": ("lagged_moments", lambda: ((_z(5, 4), 1.0), {})),
    "lagged_moments/lag_bool": ("lagged_moments", lambda: ((_z(5, 4), True), {})),
    "lagged_moments/lag_zero": ("lagged_moments", lambda: ((_z(5, 4), 0), {})),
    "lagged_moments/lag_is_frames": ("lagged_moments", lambda: ((_z(5, 4), 5), {})),
    "lagged_moments/no_frames": ("lagged_moments", lambda: ((_z(0, 4), 1), {})),
    "lagged_moments/lag_then_cpu": ("lagged_moments", lambda: ((_z(5, 4, dtype=torch.float64), 7), {})),
    "lagged_moments/cpu": ("lagged_moments", lambda: ((_z(5, 4), np.int64(2)), {})),
    "lagged_moments/cpu_float64": ("lagged_moments", lambda: ((_z(5, 4, dtype=torch.float64), 2), {})),
    "project_frames/width": ("project_frames", lambda: ((_z(5, 0), np.zeros(0), np.zeros((0, 1))), {})),
    "project_frames/mean_shape": ("project_frames", lambda: ((_z(5, 4), np.zeros(3), np.zeros((4, 2))), {})),
    "project_frames/v_shape": ("project_frames", lambda: ((_z(5, 4), np.zeros(4), np.zeros((3, 2))), {})),
    "project_frames/v_ndim": ("project_frames", lambda: ((_z(5, 4), np.zeros(4), np.zeros(4)), {})),
    "project_frames/d_zero": ("project_frames", lambda: ((_z(5, 4), np.zeros(4), np.zeros((4, 0))), {})),
    "project_frames/d_above_width": ("project_frames", lambda: ((_z(5, 4), torch.zeros(4, dtype=torch.float64), torch.zeros(4, 5, dtype=torch.float64)), {})),
    "project_frames/no_tables": ("project_frames", lambda: ((_z(5, 4), None, None), {})),
    "project_frames/shapes_then_cpu": ("project_frames", lambda: ((_z(5, 4, dtype=torch.float64), np.zeros(5), np.zeros((4, 2))), {})),
    "project_frames/cpu": ("project_frames", lambda: ((_z(5, 4), np.zeros(4), np.zeros((4, 2))), {})),
    "project_frames/cpu_then_table_dtype": ("project_frames", lambda: ((_z(5, 4), np.zeros(4, np.float32), torch.zeros(4, 2)), {})),
    "autocov_sums/ndim": ("autocov_sums", lambda: ((_z(5, 1, dtype=torch.float64), 2), {})),
    "autocov_sums/not_a_tensor": ("autocov_sums", lambda: ((np.zeros(5), 2), {})),
    "autocov_sums/ndim_then_lag": ("autocov_sums", lambda: ((_z(5, 1, dtype=torch.float64), -1), {})),
    "autocov_sums/lag_float": ("autocov_sums", lambda: ((_z(5, dtype=torch.float64), 2.0), {})),
    "autocov_sums/lag_negative": ("autocov_sums", lambda: ((_z(5, dtype=torch.float64), -1), {})),
    "autocov_sums/lag_high": ("autocov_sums", lambda: ((_z(5, dtype=torch.float64), 4097), {})),
    "autocov_sums/lag_then_cpu": ("autocov_sums", lambda: ((_z(5), False), {})),
    "autocov_sums/cpu": ("autocov_sums", lambda: ((_z(5, dtype=torch.float64), 2), {})),
    "autocov_sums/cpu_float32": ("autocov_sums", lambda: ((_z(5), 4096), {})),
    "check_centers_shape/no_centers": ("check_centers_shape", lambda: ((0, 2), {})),
    "check_centers_shape/too_many": ("check_centers_shape", lambda: ((1025, 2), {})),
    "check_centers_shape/columns": ("check_centers_shape", lambda: ((5, 129), {})),
    "check_centers_shape/product": ("check_centers_shape", lambda: ((1024, 17), {})),
    "assign_centers/ndim": ("assign_centers", lambda: ((_z(10, dtype=torch.float64), np.zeros((5, 2))), {})),
    "assign_centers/no_columns": ("assign_centers", lambda: ((_z(10, 0, dtype=torch.float64), np.zeros((5, 0))), {})),
    "assign_centers/too_wide": ("assign_centers", lambda: ((_z(10, 129, dtype=torch.float64), np.zeros((5, 129))), {})),
    "assign_centers/columns_then_centers": ("assign_centers", lambda: ((_z(10, 129, dtype=torch.float64), np.zeros((5, 2))), {})),
    "assign_centers/centers_shape": ("assign_centers", lambda: ((_z(10, 2, dtype=torch.float64), np.zeros((5, 3))), {})),
    "assign_centers/centers_ndim": ("assign_centers", lambda: ((_z(10, 2, dtype=torch.float64), np.zeros(2)), {})),
    "assign_centers/no_centers": ("assign_centers", lambda: ((_z(10, 2, dtype=torch.float64), None), {})),
    "assign_centers/centers_limit": ("assign_centers", lambda: ((_z(10, 2, dtype=torch.float64), np.zeros((1025, 2))), {})),
    "assign_centers/product": ("assign_centers", lambda: ((_z(10, 17, dtype=torch.float64), torch.zeros(1024, 17, dtype=torch.float64)), {})),
    "assign_centers/limit_then_cpu": ("assign_centers", lambda: ((_z(10, 2), np.zeros((0, 2))), {})),
    "assign_centers/cpu": ("assign_centers", lambda: ((_z(10, 2, dtype=torch.float64), np.zeros((5, 2))), {})),
    "assign_centers/cpu_float32": ("assign_centers", lambda: ((_z(10, 2), np.zeros((5, 2), np.float32)), {"n_changed": _z(1, dtype=torch.int64)})),
    "cluster_sums/ndim": ("cluster_sums", lambda: ((_z(10, 2, 2, dtype=torch.float64), _LABELS(), 5), {})),
    "cluster_sums/too_wide": ("cluster_sums", lambda: ((_z(10, 129, dtype=torch.float64), _LABELS(), 5), {})),
    "cluster_sums/columns_then_k": ("cluster_sums", lambda: ((_z(10, 129, dtype=torch.float64), _LABELS(), 5.0), {})),
    "cluster_sums/k_float": ("cluster_sums", lambda: ((_z(10, 2, dtype=torch.float64), _LABELS(), 5.0), {})),
    "cluster_sums/k_bool": ("cluster_sums", lambda: ((_z(10, dtype=torch.float64), _LABELS(), True), {})),
    "cluster_sums/k_zero": ("cluster_sums", lambda: ((_z(10, 2, dtype=torch.float64), _LABELS(), 0), {})),
    "cluster_sums/k_high": ("cluster_sums", lambda: ((_z(10, dtype=torch.float64), _LABELS(), 1025), {})),
    "cluster_sums/k_then_cpu": ("cluster_sums", lambda: ((_z(10, 2), _LABELS(), 8193), {})),
    "cluster_sums/cpu": ("cluster_sums", lambda: ((_z(10, 2, dtype=torch.float64), _LABELS(), 5), {})),
    "cluster_sums/cpu_one_column": ("cluster_sums", lambda: ((_z(10, dtype=torch.float64), _LABELS(), 5), {})),
    "transition_counts/cpu": ("transition_counts", lambda: ((_LABELS(), 1, 4), {})),
    "transition_counts/labels_then_lag": ("transition_counts", lambda: ((_LABELS(), 0, 0), {})),
    "transition_counts/int64": ("transition_counts", lambda: ((_z(10, dtype=torch.int64), 1, 4), {})),
    "label_counts/cpu": ("label_counts", lambda: ((_LABELS(), [0, 10], 4), {})),
    "label_counts/labels_then_states": ("label_counts", lambda: ((_z(10, 1, dtype=torch.int32), [10, 0], 0), {})),
    "check_swd_shapes/no_columns": ("check_swd_shapes", lambda: ((0, 4), {})),
    "check_swd_shapes/too_wide": ("check_swd_shapes", lambda: ((129, 4), {})),
    "check_swd_shapes/no_directions": ("check_swd_shapes", lambda: ((8, 0), {})),
    "check_swd_shapes/too_many_directions": ("check_swd_shapes", lambda: ((8, 65), {})),
    "swd_project/ndim": ("swd_project", lambda: ((_z(10), np.zeros((8, 4), np.float32)), {})),
    "swd_project/no_frames": ("swd_project", lambda: ((_z(0, 8), np.zeros((8, 4), np.float32)), {})),
    "swd_project/frames_then_proj": ("swd_project", lambda: ((_z(0, 8), np.zeros((7, 4), np.float32)), {})),
    "swd_project/proj_shape": ("swd_project", lambda: ((_z(10, 8), np.zeros((7, 4), np.float32)), {})),
    "swd_project/proj_ndim": ("swd_project", lambda: ((_z(10, 8), np.zeros(8, np.float32)), {})),
    "swd_project/too_wide": ("swd_project", lambda: ((_z(10, 129), np.zeros((129, 4), np.float32)), {})),
    "swd_project/directions": ("swd_project", lambda: ((_z(10, 8), torch.zeros(8, 65)), {})),
    "swd_project/limits_then_dtype": ("swd_project", lambda: ((_z(10, 8), np.zeros((8, 0))), {})),
    "swd_project/proj_float64": ("swd_project", lambda: ((_z(10, 8), np.zeros((8, 4))), {})),
    "swd_project/proj_tensor_float64": ("swd_project", lambda: ((_z(10, 8), torch.zeros(8, 4, dtype=torch.float64)), {})),
    "swd_project/dtype_then_cpu": ("swd_project", lambda: ((_z(10, 8, dtype=torch.float64), np.zeros((8, 4))), {})),
    "swd_project/cpu": ("swd_project", lambda: ((_z(10, 8), np.zeros((8, 4), np.float32)), {})),
    "swd_sort_segments/ndim": ("swd_sort_segments", lambda: ((_z(10), [10]), {})),
    "swd_sort_segments/no_keys": ("swd_sort_segments", lambda: ((_z(4, 0), [1]), {})),
    "swd_sort_segments/directions": ("swd_sort_segments", lambda: ((_z(65, 10), [10]), {})),
    "swd_sort_segments/keys_then_cuts": ("swd_sort_segments", lambda: ((_z(0, 10), [11]), {})),
    "swd_sort_segments/cuts": ("swd_sort_segments", lambda: ((_z(4, 10), [5, 11]), {})),
    "swd_sort_segments/cuts_float": ("swd_sort_segments", lambda: ((_z(4, 10), [5.0]), {})),
    "swd_sort_segments/cuts_then_cpu": ("swd_sort_segments", lambda: ((_z(4, 10, dtype=torch.float64), []), {})),
    "swd_sort_segments/cpu": ("swd_sort_segments", lambda: ((_z(4, 10), [5, 10]), {})),
    "swd_merge/a_ndim": ("swd_merge", lambda: ((_z(10), _z(4, 10)), {})),
    "swd_merge/b_no_keys": ("swd_merge", lambda: ((_z(4, 10), _z(4, 0)), {})),
    "swd_merge/a_then_b": ("swd_merge", lambda: ((_z(65, 10), _z(4, 0)), {})),
    "swd_merge/directions_differ": ("swd_merge", lambda: ((_z(4, 10), _z(3, 10)), {})),
    "swd_merge/differ_then_cpu": ("swd_merge", lambda: ((_z(4, 10, dtype=torch.float64), _z(3, 10)), {})),
    "swd_merge/cpu": ("swd_merge", lambda: ((_z(4, 10), _z(4, 6)), {})),
    "swd_w2sq/u_ndim": ("swd_w2sq", lambda: ((_z(4, 10, 1), _z(4, 10)), {})),
    "swd_w2sq/v_not_a_tensor": ("swd_w2sq", lambda: ((_z(4, 10), np.zeros((4, 10), np.float32)), {})),
    "swd_w2sq/u_then_v": ("swd_w2sq", lambda: ((_z(0, 10), _z(65, 10)), {})),
    "swd_w2sq/directions_differ": ("swd_w2sq", lambda: ((_z(4, 10), _z(5, 10)), {})),
    "swd_w2sq/differ_then_cpu": ("swd_w2sq", lambda: ((_z(4, 10, dtype=torch.float64), _z(5, 10)), {})),
    "swd_w2sq/cpu": ("swd_w2sq", lambda: ((_z(4, 10), _z(4, 6)), {})),
    "_state_map/n_states_float": ("_state_map", lambda: ((None, 4.0, "cpu"), {})),
    "_state_map/n_states_bool": ("_state_map", lambda: ((None, True, "cpu"), {})),
    "_state_map/n_states_str": ("_state_map", lambda: ((None, "4", "cpu"), {})),
    "_state_map/n_states_zero": ("_state_map", lambda: (([0, 1], 0, "cpu"), {})),
    "_state_map/n_states_high": ("_state_map", lambda: ((None, 1025, "cpu"), {})),
    "_state_map/n_states_then_map": ("_state_map", lambda: ((_z(2, 2, dtype=torch.int64), -1, "cpu"), {})),
    "_state_map/map_int64_tensor": ("_state_map", lambda: ((_z(3, dtype=torch.int64), 4, "cpu"), {})),
    "_state_map/map_float_tensor": ("_state_map", lambda: ((_z(3), 4, "cpu"), {})),
    "_state_map/map_two_dims": ("_state_map", lambda: ((_z(2, 3, dtype=torch.int32), 4, "cpu"), {})),
    "_state_map/map_two_dims_host": ("_state_map", lambda: (([[0, 1], [2, 3]], 4, "cpu"), {})),
    "_state_map/map_empty": ("_state_map", lambda: ((_z(0, dtype=torch.int32), 4, "cpu"), {})),
    "_state_map/map_empty_host": ("_state_map", lambda: (([], 4, "cpu"), {})),
    "_state_map/map_scalar_tensor": ("_state_map", lambda: ((torch.tensor(3, dtype=torch.int32), 4, "cpu"), {})),
    "_result/shape": ("_result", lambda: (("out", _z(2, 3), (2, 4), torch.float32, torch.device("cpu")), {})),
    "_result/dtype": ("_result", lambda: (("sums", _z(2, 3), (2, 3), torch.float64, torch.device("cpu")), {})),
    "_result/strided": ("_result", lambda: (("out", _z(3, 2).t(), (2, 3), torch.float32, torch.device("cpu")), {"fill": 0})),
    "_result/device": ("_result", lambda: (("rmsd", _z(2), (2,), torch.float32, torch.device("meta")), {})),
    "_table/dtype": ("_table", lambda: (("an index table", "int32 [F, 4]", _z(2, 4, dtype=torch.int64), True, torch.device("cpu"), torch.int32, (None, 4)), {})),
    "_table/shape": ("_table", lambda: (("bounds", "int32 [n_seg + 1]", _z(2, 4, dtype=torch.int32), True, torch.device("cpu"), torch.int32, (None,)), {})),
}


def py_answer(native, fn: str, make) -> dict:
    """One call of a Python entry point -> ``{"raises", "text"}`` (``raises`` is None if it returned)."""
    args, kwargs = make()
    try:
        getattr(native, fn)(*args, **kwargs)
    except Exception as e:  # noqa: BLE001 (the class is what the table records)
        return {"raises": type(e).__name__, "text": str(e)}
    return {"raises": None, "text": ""}


def answers() -> dict:
    """Every case of both parts, answered by the tree this runs in."""
    from jamun_amd import _lib, native

    lib = _lib.load()
    got = {name: c_answer(lib, entry, args) for name, (entry, args) in C_CASES.items()}
    got.update({name: py_answer(native, fn, make) for name, (fn, make) in PY_CASES.items()})
    return got
