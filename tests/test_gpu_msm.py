"""GPU tests of jamun_msm.hip (nearest centres, cluster sums, transition and occupancy counts), of k-means on the device and of the MSM meter
on the device path.  The expected values are the host specification's (jamun_amd/msm.py, pinned against double loops in test_msm_host.py)
on the same float64 input: labels and counts integer for integer, distances and sums bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _msm_cases as mc
from _frames_common import _dev, guarded, intact, meter_run, tree
from _traj_molecules import dipeptide
from jamun_amd import msm

pytestmark = pytest.mark.gpu

SENTINEL = -77
FRAMES = [1, 63, 64, 65, 1023, 1024, 1025, 2049]  # around a wave, around a slice of the sums, two slices and one frame
KS = [1, 2, 64, 65, 100, 128]


def _strided(y: np.ndarray, dev, extra: int = 3) -> torch.Tensor:
    """The rows ``y`` as a view of a wider block whose other columns hold NaN (row_stride > d)."""
    T, d = y.shape
    wide = torch.full((T, d + extra), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :d] = torch.from_numpy(np.array(y)).to(dev)
    return wide[:, :d]


def _check_assign_and_sums(y: np.ndarray, centers: np.ndarray, frames, dev):
    from jamun_amd import native

    k, d = centers.shape
    want_l, want_s = msm.assign_centers_host(y, centers)  # (a row's label does not depend on the other rows: prefixes share it)
    c_dev = torch.from_numpy(centers).to(dev)
    for T in frames:
        what = (T, d, k)
        for view in (_strided(y[:T], dev), torch.from_numpy(np.array(y[:T])).to(dev)) if T in (65, 2049) else (_strided(y[:T], dev),):
            big_l, out_l = guarded((T,), dev, torch.int32, SENTINEL)
            big_s, out_s = guarded((T,), dev, torch.float64, float(SENTINEL))
            labels, sq, _ = native.assign_centers(view, c_dev, labels=out_l, sqdist=out_s)
            torch.cuda.synchronize()
            assert labels.data_ptr() == out_l.data_ptr() and intact(big_l, SENTINEL) and intact(big_s, float(SENTINEL)), what
            assert np.array_equal(labels.cpu().numpy(), want_l[:T]) and np.array_equal(sq.cpu().numpy(), want_s[:T]), what
            again_l, again_s, _ = native.assign_centers(view, c_dev, sqdist=True)
            assert torch.equal(again_l, labels) and torch.equal(again_s, sq), what
            mixed = mc.labels_with_outliers(T, k, seed=d)  # labels of any kind, -1 and out-of-range values among them
            for lab in (want_l[:T], mixed):
                want_c, want_sum = msm.cluster_sums_host(y[:T], lab, k)
                big_c, out_c = guarded((k,), dev, torch.int64, SENTINEL)
                big_m, out_m = guarded((k, d), dev, torch.float64, float(SENTINEL))
                lab_dev = torch.from_numpy(lab).to(dev)
                counts, sums = native.cluster_sums(view, lab_dev, k, counts=out_c, sums=out_m)
                torch.cuda.synchronize()
                assert intact(big_c, SENTINEL) and intact(big_m, float(SENTINEL)), what
                assert np.array_equal(counts.cpu().numpy(), want_c) and np.array_equal(sums.cpu().numpy(), want_sum), what
                again_c, again_m = native.cluster_sums(view, lab_dev, k)
                assert torch.equal(again_c, counts) and torch.equal(again_m, sums), what
            inertia = native.cluster_sums(sq, labels, k)[1].cpu().numpy()  # d = 1 on the distances: the inertia of every cluster
            assert np.array_equal(inertia, msm.cluster_sums_host(want_s[:T], want_l[:T], k)[1]), what


@pytest.mark.parametrize("d", [1, 2, 3, 17, 128])
def test_assignment_and_cluster_sums_equal_the_host_specification_bit_for_bit(d):
    dev = _dev()
    y = mc.projection_rows(max(FRAMES), d)
    for k in KS:
        frames = FRAMES if k in (2, 100) or d == 128 and k == 128 else [65, 1025]
        _check_assign_and_sums(y, mc.centers_for(y, k, seed=d), frames, dev)


def test_the_corner_of_1024_centres_of_16_columns_goes_through_the_tiles():
    dev = _dev()
    y = mc.projection_rows(1025, 16)
    _check_assign_and_sums(y, mc.centers_for(y, 1024), [1, 1025], dev)
    y = mc.projection_rows(300, 128)  # 128 columns: tiles of 32 centres, four tiles and a fifth of one centre
    _check_assign_and_sums(y, mc.centers_for(y, 128, seed=3)[:127], [300], dev)


def test_frozen_fma_sensitive_frames_and_exact_ties_get_the_specifications_labels():
    from jamun_amd import native

    dev = _dev()
    for d in (3, 17):
        for y, c, spec_label, fused_label in mc.fma_cases(d):
            labels, sq, _ = native.assign_centers(torch.from_numpy(np.array(y)).to(dev), np.array(c), sqdist=True)
            assert int(labels.item()) == spec_label != fused_label, (d, spec_label)
            assert float(sq.item()) == mc.spec_distance(y[0], c[spec_label])
    labels, sq, _ = native.assign_centers(torch.from_numpy(np.array(mc.TIE_FRAMES)).to(dev), np.array(mc.TIE_CENTERS), sqdist=True)
    assert np.array_equal(labels.cpu().numpy(), mc.TIE_LABELS) and np.array_equal(sq.cpu().numpy(), msm.assign_centers_host(mc.TIE_FRAMES, mc.TIE_CENTERS)[1])


def test_a_non_finite_row_gets_minus_one_and_disturbs_no_other_and_n_changed_counts():
    from jamun_amd import native

    dev = _dev()
    for d in (3, 17):
        T, k = 1025, 5
        y = np.array(mc.projection_rows(T, d))
        c = mc.centers_for(y, k)
        clean_l, clean_s = msm.assign_centers_host(y, c)
        y[0, 0], y[64, d - 1], y[1024, 1] = np.nan, np.inf, -np.inf
        want_l, want_s = msm.assign_centers_host(y, c)
        y_dev = torch.from_numpy(y).to(dev)
        labels, sq, _ = native.assign_centers(y_dev, c, sqdist=True)
        bad = np.array([0, 64, 1024])
        others = np.setdiff1d(np.arange(T), bad)
        got_l, got_s = labels.cpu().numpy(), sq.cpu().numpy()
        assert (got_l[bad] == -1).all() and np.isnan(got_s[bad]).all() and np.array_equal(got_l, want_l) and np.array_equal(got_s, want_s, equal_nan=True)
        assert np.array_equal(got_l[others], clean_l[others]) and np.array_equal(got_s[others], clean_s[others])
        # n_changed: against other labels, against the result itself (0), added to what the counter holds, and in place
        prev = mc.labels_with_outliers(T, k, seed=9)
        _, _, n = native.assign_centers(y_dev, c, prev_labels=torch.from_numpy(prev).to(dev))
        assert n.dtype == torch.int64 and int(n.item()) == int(np.count_nonzero(prev != want_l)) > 0
        _, _, n0 = native.assign_centers(y_dev, c, prev_labels=labels)
        assert int(n0.item()) == 0
        _, _, n = native.assign_centers(y_dev, c, prev_labels=torch.from_numpy(prev).to(dev), n_changed=n)
        assert int(n.item()) == 2 * int(np.count_nonzero(prev != want_l))
        same = torch.from_numpy(prev).to(dev)
        out, _, n = native.assign_centers(y_dev, c, labels=same, prev_labels=same)
        assert out.data_ptr() == same.data_ptr() and np.array_equal(same.cpu().numpy(), want_l) and int(n.item()) == int(np.count_nonzero(prev != want_l))


@pytest.mark.parametrize("n_states", [1, 3, 10, 100, 1024])
def test_transition_and_label_counts_equal_the_host_specification(n_states):
    from jamun_amd import native

    dev = _dev()
    rng = np.random.RandomState(n_states)
    n_in = n_states + 13
    state_map = rng.randint(-1, n_states + 1, size=n_in).astype(np.int32)  # (-1 and n_states: none)
    for T in (1, 65, 1025, 4097 if n_states in (3, 1024) else 2049):
        for smap in (None, state_map):
            labels = mc.labels_with_outliers(T, n_in if smap is not None else n_states, seed=3)
            lab_dev = torch.from_numpy(labels).to(dev)
            for lag in sorted({1, 2, max(T - 1, 1), T}):
                what = (n_states, T, smap is not None, lag)
                want = msm.transition_counts_host(labels, lag, n_states, smap)
                big, out = guarded((n_states, n_states), dev, torch.int64, 0)
                got = native.transition_counts(lab_dev, lag, n_states, state_map=smap, out=out)
                torch.cuda.synchronize()
                assert got.data_ptr() == out.data_ptr() and intact(big, 0) and np.array_equal(got.cpu().numpy(), want), what
                assert lag < T or not want.any(), what
                native.transition_counts(lab_dev, lag, n_states, state_map=smap, out=out)  # a second call adds onto the first
                assert np.array_equal(out.cpu().numpy(), 2 * want) and intact(big, 0), what
            cuts = np.unique(rng.randint(0, T + 1, size=6))
            bounds = np.sort(np.concatenate([[0, 0], cuts, cuts[:2], [T]])).astype(np.int32)  # empty segments among them
            want = msm.label_counts_host(labels, bounds, n_states, smap)
            big, out = guarded((bounds.shape[0] - 1, n_states), dev, torch.int64, 0)
            got = native.label_counts(lab_dev, bounds, n_states, state_map=smap, out=out)
            torch.cuda.synchronize()
            assert intact(big, 0) and np.array_equal(got.cpu().numpy(), want), (n_states, T, smap is not None)
            assert want.sum() == (msm.states_host(labels, n_states, smap) >= 0).sum()
            native.label_counts(lab_dev, torch.from_numpy(bounds).to(dev), n_states, state_map=smap, out=out)
            assert np.array_equal(out.cpu().numpy(), 2 * want) and intact(big, 0)
            inner = np.array([min(2, T), max(T - 1, min(2, T))], dtype=np.int32)  # frames before the first bound and behind the last count nowhere
            assert np.array_equal(native.label_counts(lab_dev, inner, n_states, state_map=smap).cpu().numpy(), msm.label_counts_host(labels, inner, n_states, smap))


def test_the_c_entries_refuse_bad_arguments_and_write_nothing():
    from jamun_amd import _lib

    dev = _dev()
    lib = _lib.load()
    T, d, k, n, S = 70, 3, 4, 5, 3
    y = torch.from_numpy(np.array(mc.projection_rows(T, d))).to(dev)
    c = torch.from_numpy(mc.centers_for(mc.projection_rows(T, d), k)).to(dev)
    prev = torch.zeros(T, dtype=torch.int32, device=dev)
    smap = torch.arange(n, dtype=torch.int32, device=dev)
    bounds = torch.tensor([0, 10, 10, T], dtype=torch.int32, device=dev)
    big_l, labels = guarded((T,), dev, torch.int32, SENTINEL)
    big_q, sq = guarded((T,), dev, torch.float64, float(SENTINEL))
    big_n, changed = guarded((1,), dev, torch.int64, SENTINEL)
    big_c, counts = guarded((k,), dev, torch.int64, SENTINEL)
    big_s, sums = guarded((k, d), dev, torch.float64, float(SENTINEL))
    big_w, work = guarded((k * d + k,), dev, torch.float64, float(SENTINEL))
    big_t, trans = guarded((n, n), dev, torch.int64, SENTINEL)
    big_o, occ = guarded((S, n), dev, torch.int64, SENTINEL)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda a: None if a is None else a.data_ptr()
    err = lib.jamun_last_error

    def asg(n_frames=T, dd=d, kk=k, stride=d, ys=y, cs=c, l=labels, q=sq, pv=prev, nc=changed):
        return lib.jamun_assign_centers(p(ys), stride, n_frames, dd, p(cs), kk, p(l), p(q), p(pv), p(nc), st)

    def cls(n_frames=T, dd=d, kk=k, stride=d, ys=y, l=prev, cn=counts, sm=sums, w=work, cap=None):
        return lib.jamun_cluster_sums(p(ys), stride, n_frames, dd, p(l), kk, p(cn), p(sm), p(w), work.numel() if cap is None else cap, st)

    def trn(n_frames=T, lag=2, l=prev, m=smap, n_in=n, ns=n, o=trans):
        return lib.jamun_transition_counts(p(l), n_frames, lag, p(m), n_in, ns, p(o), st)

    def occf(n_frames=T, l=prev, m=smap, n_in=n, ns=n, b=bounds, seg=S, o=occ):
        return lib.jamun_label_counts(p(l), n_frames, p(m), n_in, ns, p(b), seg, p(o), st)

    need = C.c_int64(-1)
    assert lib.jamun_cluster_sums_work(T, d, k, C.byref(need)) == 0 and need.value == k * d + k
    assert lib.jamun_cluster_sums_work(2049, 128, 128, C.byref(need)) == 0 and need.value == 3 * (128 * 128 + 128)
    assert lib.jamun_cluster_sums_work(0, d, k, C.byref(need)) == 0 and need.value == 0
    assert lib.jamun_cluster_sums_work(T, d, 1025, C.byref(need)) == -1 and lib.jamun_cluster_sums_work(-1, d, k, C.byref(need)) == -1
    assert lib.jamun_cluster_sums_work(T, d, k, None) == -1 and b"null" in err()
    for call in (asg, cls):
        assert call(kk=0) == -1 and call(kk=1025) == -1 and b"k " in err()
        assert call(dd=0) == -1 and call(dd=129) == -1 and b"d " in err()
        assert call(kk=129, dd=128) == -1 and b"k * d" in err()
        assert call(stride=d - 1) == -1 and b"row_stride" in err()
        assert call(n_frames=-1) == -1 and call(stride=-1) == -1 and b"negative" in err()
    for null in ("ys", "cs", "l"):
        assert asg(**{null: None}) == -1 and b"null" in err(), null
    assert asg(pv=None) == -1 and asg(nc=None) == -1 and b"go together" in err()
    assert cls(cap=k * d + k - 1) == -1 and b"work_capacity" in err() and cls(cap=-1) == -1
    for null in ("ys", "l", "cn", "sm", "w"):
        assert cls(**{null: None}) == -1 and b"null" in err(), null
    for call in (trn, occf):
        assert call(ns=0) == -1 and call(ns=1025) == -1 and b"n_states" in err()
        assert call(n_in=0) == -1 and b"n_in" in err()
        assert call(n_frames=-1) == -1 and b"negative" in err()
        assert call(l=None) == -1 and call(o=None) == -1 and b"null" in err()
    assert trn(lag=0) == -1 and trn(lag=-3) == -1 and b"lag" in err()
    assert occf(seg=0) == -1 and occf(seg=4097) == -1 and b"n_seg" in err()
    assert occf(b=None) == -1 and b"null" in err()
    # no frames (or no pair that far apart): nothing is launched, null pointers pass
    assert asg(n_frames=0) == 0 and asg(n_frames=0, ys=None, cs=None, l=None, q=None, pv=None, nc=None) == 0
    assert cls(n_frames=0) == 0 and cls(n_frames=0, ys=None, l=None, cn=None, sm=None, w=None, cap=0) == 0
    assert trn(n_frames=0) == 0 and trn(lag=T) == 0 and trn(lag=T, l=None, o=None) == 0 and occf(n_frames=0, l=None, b=None, o=None) == 0
    torch.cuda.synchronize()
    for big, fill in ((big_l, SENTINEL), (big_q, float(SENTINEL)), (big_n, SENTINEL), (big_c, SENTINEL), (big_s, float(SENTINEL)), (big_w, float(SENTINEL)),
                      (big_t, SENTINEL), (big_o, SENTINEL)):
        assert (big == fill).all()
    # and the same buffers take the results of good calls, the pads intact
    changed.zero_(), trans.zero_(), occ.zero_()
    assert asg() == 0 and asg(q=None, pv=None, nc=None) == 0
    torch.cuda.synchronize()
    want_l, want_q = msm.assign_centers_host(y.cpu().numpy(), c.cpu().numpy())
    assert np.array_equal(labels.cpu().numpy(), want_l) and np.array_equal(sq.cpu().numpy(), want_q) and int(changed.item()) == np.count_nonzero(want_l)
    prev.copy_(labels)
    assert cls() == 0 and trn() == 0 and trn(m=None, n_in=-5) == 0 and occf() == 0
    torch.cuda.synchronize()
    want_c, want_s = msm.cluster_sums_host(y.cpu().numpy(), want_l, k)
    assert np.array_equal(counts.cpu().numpy(), want_c) and np.array_equal(sums.cpu().numpy(), want_s)
    assert np.array_equal(trans.cpu().numpy(), 2 * msm.transition_counts_host(want_l, 2, n))  # (the identity map and no map: the same counts twice)
    assert np.array_equal(occ.cpu().numpy(), msm.label_counts_host(want_l, [0, 10, 10, T], n))
    for big, fill in ((big_l, SENTINEL), (big_q, float(SENTINEL)), (big_n, SENTINEL), (big_c, SENTINEL), (big_s, float(SENTINEL)), (big_w, float(SENTINEL)),
                      (big_t, SENTINEL), (big_o, SENTINEL)):
        assert intact(big, fill)


def test_the_count_bindings_refuse_what_only_labels_on_a_gpu_let_them_reach():
    """`native.transition_counts` and `native.label_counts` check their labels first, and those must be on a GPU: the refusals behind that
    check (``lag``, ``n_states``, ``state_map``, ``bounds``, the segment count, ``out=``), their texts and which of two faults is reported.
    Every call is refused on the host: nothing is launched."""
    import re

    from jamun_amd import native

    dev = _dev()
    T = 20
    labels = torch.zeros(T, dtype=torch.int32, device=dev)

    def refused(kind, text, fn, *args, **kwargs):
        with pytest.raises(kind, match="^" + re.escape(text) + "$"):
            fn(*args, **kwargs)

    for lag in (0, -2, 1.0, True, "1"):
        refused(ValueError, f"lag must be an integer of at least 1, got {lag!r}", native.transition_counts, labels, lag, 4)
    refused(RuntimeError, "lag must fit 31 bits", native.transition_counts, labels, 2**31, 4)
    refused(RuntimeError, f"labels must be a contiguous int32 [frames] tensor on the GPU, got torch.int64 ({T},) on {dev}",
            native.transition_counts, labels.long(), 0, 0)  # (labels, then lag)
    refused(ValueError, "lag must be an integer of at least 1, got 0", native.transition_counts, labels, 0, 0)  # (lag, then n_states)
    for fn, mid in ((native.transition_counts, 1), (native.label_counts, [0, T])):
        for n_states in (0, 1025, 4.0, False):
            refused(ValueError, f"n_states must be an integer in [1, 1024], got {n_states!r}", fn, labels, mid, n_states)
        refused(ValueError, "state_map must be a non-empty int32 [n_in] table, got torch.int64 (3,)", fn, labels, mid, 4,
                state_map=torch.zeros(3, dtype=torch.int64, device=dev))
        refused(ValueError, "state_map must be a non-empty int32 [n_in] table, got torch.int32 (0,)", fn, labels, mid, 4, state_map=[])
    refused(RuntimeError, f"out must be a contiguous int64 [4, 4] tensor on {dev}, got torch.int32 (4, 4) on {dev}", native.transition_counts, labels, 1, 4,
            out=torch.zeros(4, 4, dtype=torch.int32, device=dev))
    for bounds, shown in (([0], "[0]"), ([5, 3], "[5, 3]"), ([0, T + 1], f"[0, {T + 1}]"), ([-1, 5], "[-1, 5]"), ([0.0, 5.0], "[0.0, 5.0]"),
                          ([[0, 5]], "[[0, 5]]"), (np.arange(17)[::-1], "(17,)")):
        refused(ValueError, f"bounds must be at least two non-decreasing integers within [0, {T}], got {shown}", native.label_counts, labels, bounds, 4)
    refused(ValueError, "n_states must be an integer in [1, 1024], got 0", native.label_counts, labels, [5, 3], 0)  # (n_states, then bounds)
    refused(ValueError, f"bounds on the device must be a contiguous int32 [n_seg + 1] tensor on {dev}, got torch.int64 (3,) on {dev}",
            native.label_counts, labels, torch.tensor([0, 5, T], device=dev), 4)
    refused(ValueError, "4097 segments: the device path takes 1 to 4096", native.label_counts, labels, np.zeros(4098, np.int64), 4)
    refused(ValueError, "0 segments: the device path takes 1 to 4096", native.label_counts, labels, torch.zeros(1, dtype=torch.int32, device=dev), 4)
    refused(RuntimeError, f"out must be a contiguous int64 [2, 4] tensor on {dev}, got torch.int64 (4, 2) on {dev}", native.label_counts, labels, [0, 5, T], 4,
            out=torch.zeros(4, 2, dtype=torch.int64, device=dev))


@pytest.mark.parametrize("T,d,k", [(2049, 2, 8), (1500, 17, 65)])
def test_kmeans_on_the_device_gives_the_hosts_centres_bit_for_bit(T, d, k):
    dev = _dev()
    y = mc.projection_rows(T, d, seed=4)
    y_dev = _strided(y, dev)
    c0 = msm.kmeans_init_host(y_dev, k)
    assert np.array_equal(c0, msm.kmeans_init_host(y, k))  # the subsample comes from the device unchanged
    host, device = msm.kmeans(y, c0, max_iter=30), msm.kmeans(y_dev, c0, max_iter=30)
    assert torch.is_tensor(device["labels"]) and device["labels"].is_cuda and host["n_iter"] > 2
    assert device["n_iter"] == host["n_iter"] and device["converged"] == host["converged"]
    assert np.array_equal(device["centers"], host["centers"]) and device["inertia"] == host["inertia"]
    assert np.array_equal(device["labels"].cpu().numpy(), host["labels"]) and np.array_equal(device["counts"], host["counts"])


# ---- the meter on the device path ------------------------------------------------------------------------------------------------------------------------------------

def _kernel_features(meter, dev):
    """The meter's features from jamun_intcoord.hip whatever path the meter is on (as in test_gpu_tica.py: the two paths' own features differ
    in the last bits of fp32, which is test_gpu_intcoord.py's subject; the comparison below starts from the same feature rows)."""
    from jamun_amd import native

    index = torch.from_numpy(meter.index).to(dev)

    def features(frames):
        frames = frames if torch.is_tensor(frames) else torch.from_numpy(np.asarray(frames))
        return native.internal_coords(frames.to(dev), index, cossin=True).cpu().numpy()

    return features


def test_meter_on_device_tensors_agrees_with_the_host_path(tmp_path):
    """The fixture of test_msm_host.py (psi hopping between three wells; 3000 reference frames, two batches of three chains of 400).  Every
    integer output is equal; the floats lie within `_msm_cases.TOLERANCE`: ten times what moving every projected value by the TICA
    tolerance did on the CPU, which is 0 for everything computed from counts alone.  A second device run writes the same bytes."""
    from jamun_amd.callbacks import MSMMetricsCallback

    dev = _dev()
    mol = dipeptide()
    ref, batches = mc.meter_fixture(mol, dev)
    device_cb, device_smp = meter_run(MSMMetricsCallback, tmp_path / "device", mol, batches, dev, xyz=ref, device="device", **mc.METER_KW)

    class HostOnKernelFeatures(MSMMetricsCallback):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            for meter in self.meters.values():
                meter._features = _kernel_features(meter, dev)

    host_cb, host_smp = meter_run(HostOnKernelFeatures, tmp_path / "host", mol, batches, dev, xyz=ref, device="host", **mc.METER_KW)
    assert device_cb.meters["m"]._dev and not host_cb.meters["m"]._dev
    assert all(torch.is_tensor(r["labels"]) and r["labels"].is_cuda for r in device_cb.meters["m"]._records)
    dd, hd = tmp_path / "device" / "m" / "msm", tmp_path / "host" / "m" / "msm"
    assert sorted(os.listdir(dd)) == sorted(os.listdir(hd)) == sorted([f"{i}.npz" for i in range(6)] + ["joined.npz", "model.json", "model.npz", "true_traj.npz"])
    assert open(dd / "model.json").read() == open(hd / "model.json").read()
    worst = mc.compare_outputs(mc.meter_outputs(dd), mc.meter_outputs(hd))  # (asserts every integer output equal)
    print("device path against host path, largest differences:", worst, "tolerances:", mc.TOLERANCE)
    for k, v in worst.items():
        assert v <= mc.TOLERANCE[k], (k, v, mc.TOLERANCE[k])
    assert device_smp.fabric.logged == host_smp.fabric.logged and len(device_smp.fabric.logged) == 2
    meter_run(MSMMetricsCallback, tmp_path / "again", mol, batches, dev, xyz=ref, device="device", **mc.METER_KW)
    assert tree(str(dd)) == tree(str(tmp_path / "again" / "m" / "msm"))
