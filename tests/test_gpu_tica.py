"""GPU tests of jamun_tica.hip (lagged moments, projection, autocovariance sums) and of the TICA meter on the device path.  The expected values
are the host specification's (jamun_amd/tica.py, pinned in test_tica_host.py); every tolerance is the rounding bound of the sum in question,
computed in the test from the same inputs (_tica_cases.py: any order of the additions lies within it), taken twice because the expected
value is itself such a sum in another order."""
import os

import numpy as np
import pytest
import torch

import _tica_cases as tc
from _frames_common import _dev, guarded, intact, meter_run
from _traj_molecules import dipeptide
from jamun_amd import tica

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
SLICE, TILE = 1024, 32  # the seams of the kernels as built (test_tica_host.py checks that native mirrors the header)
WIDTHS = [1, 2, 15, 16, 17, 33, 128]
# (frames, lag): one pair; around a wave of pairs; lag = 1 and lag = T - 1; one slice of pairs less one, exactly, plus one; two slices plus one
SHAPES = [(2, 1), (64, 1), (65, 1), (66, 1), (65, 64), (70, 5), (SLICE, 1), (SLICE + 1, 1), (SLICE + 2, 1), (SLICE + 7, 8), (2 * SLICE + 4, 3)]


def _strided(x: np.ndarray, dev, extra: int = 5) -> torch.Tensor:
    """The rows ``x`` as a view of a wider block whose other columns hold NaN."""
    T, W = x.shape
    wide = torch.full((T, W + extra), float("nan"), dtype=torch.float32, device=dev)
    wide[:, :W] = torch.from_numpy(np.array(x)).to(dev)
    return wide[:, :W]


@pytest.mark.parametrize("W", WIDTHS)
def test_lagged_moments_lie_within_the_rounding_bound_of_the_host_specification(W):
    from jamun_amd import native

    dev = _dev()
    assert (native.TICA_SLICE, native.TICA_TILE) == (SLICE, TILE)
    for T, lag in SHAPES:
        x = tc.feature_rows(T, W)
        want_s, want_m = tica.lagged_moments_host(x, lag)
        bound_s, bound_m = tc.moments_bounds(x, lag)
        for name, view in (("contiguous", torch.from_numpy(np.array(x)).to(dev)), ("strided", _strided(x, dev))):
            big_s, out_s = guarded((2, W), dev, torch.float64, SENTINEL)
            big_m, out_m = guarded((3, W, W), dev, torch.float64, SENTINEL)
            s, m = native.lagged_moments(view, lag, sums=out_s, moments=out_m)
            torch.cuda.synchronize()
            what = (W, T, lag, name)
            assert s.data_ptr() == out_s.data_ptr() and m.data_ptr() == out_m.data_ptr() and intact(big_s, SENTINEL) and intact(big_m, SENTINEL), what
            s, m = s.cpu().numpy(), m.cpu().numpy()
            err_s, err_m = np.abs(s - want_s), np.abs(m - want_m)
            assert (err_s <= 2 * bound_s).all(), (what, float((err_s / bound_s).max()))
            assert (err_m <= 2 * bound_m).all(), (what, float((err_m / bound_m).max()))
            assert np.array_equal(m[0], m[0].T) and np.array_equal(m[1], m[1].T), what  # G and H: symmetric bit for bit
            assert W == 1 or T - lag < 3 or not np.array_equal(m[2], m[2].T), what   # K is not symmetrised
            again_s, again_m = native.lagged_moments(view, lag)
            assert np.array_equal(again_s.cpu().numpy(), s) and np.array_equal(again_m.cpu().numpy(), m), what  # the same bits in every run


def test_lagged_moments_propagate_non_finite_values_by_ieee_rules():
    from jamun_amd import native

    dev = _dev()
    T, W, lag = SLICE + 40, 17, 3
    x = np.array(tc.feature_rows(T, W))
    x[5, 2], x[T - 1, 4], x[SLICE + 10, 16] = np.nan, np.inf, -np.inf  # (the last frame is an x_{t+lag} only; the third lies in the second slice)
    want_s, want_m = tica.lagged_moments_host(x, lag)
    s, m = native.lagged_moments(torch.from_numpy(x).to(dev), lag)
    s, m = s.cpu().numpy(), m.cpu().numpy()
    assert np.array_equal(np.isnan(s), np.isnan(want_s)) and np.array_equal(np.isnan(m), np.isnan(want_m))
    assert np.array_equal(np.isinf(s), np.isinf(want_s)) and np.array_equal(np.isinf(m), np.isinf(want_m))
    assert np.array_equal(np.sign(s[np.isinf(s)]), np.sign(want_s[np.isinf(want_s)]))
    fin = np.isfinite(want_m)
    assert fin.any() and (~fin).any() and not np.isfinite(s[1, 4]) and np.isfinite(s[0, 4])  # (the last frame is no x_t)
    clean_s, clean_m = tc.moments_bounds(np.where(np.isfinite(x), x, 0).astype(np.float32), lag)
    assert (np.abs(m[fin] - want_m[fin]) <= 2 * clean_m[fin]).all()


@pytest.mark.parametrize("W", WIDTHS)
def test_projection_lies_within_the_rounding_bound_and_a_nan_touches_its_own_row_only(W):
    from jamun_amd import native

    dev = _dev()
    rng = np.random.RandomState(W)
    for T in (1, 64, 65, SLICE + 1):
        x = tc.feature_rows(T, W, seed=1)
        for d in sorted({1, min(2, W), W}):
            mean, v = x.astype(np.float64).mean(0) + 0.01 * rng.randn(W), rng.randn(W, d) * np.array([1.0, 1e-2, 30.0])[np.arange(d) % 3]
            want, bound = tica.project_host(x, mean, v), tc.projection_bound(x, mean, v)
            for name, view in (("contiguous", torch.from_numpy(np.array(x)).to(dev)), ("strided", _strided(x, dev))):
                big, out = guarded((T, d), dev, torch.float64, SENTINEL)
                got = native.project_frames(view, mean, v, out=out)
                torch.cuda.synchronize()
                what = (W, T, d, name)
                assert got.data_ptr() == out.data_ptr() and intact(big, SENTINEL), what
                err = np.abs(got.cpu().numpy() - want)
                assert (err <= 2 * bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))
            if T >= 64:
                clean = got.cpu().numpy()
                for value, (t, j) in ((np.nan, (0, 0)), (np.inf, (63, W - 1)), (-np.inf, (T - 1, W // 2))):
                    y = np.array(x)
                    y[t, j] = value
                    dirty = native.project_frames(torch.from_numpy(y).to(dev), torch.from_numpy(mean).to(dev), torch.from_numpy(v).to(dev)).cpu().numpy()
                    others = np.arange(T) != t
                    assert not np.isfinite(dirty[t]).any() and np.array_equal(dirty[others], clean[others]), (W, T, d, value, t)


@pytest.mark.parametrize("T", [1, 2, 65, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 3])
def test_autocov_sums_lie_within_the_rounding_bound_with_zeros_behind_the_last_lag(T):
    from jamun_amd import native

    dev = _dev()
    rng = np.random.RandomState(T)
    y = rng.randn(T) * 2.0 + 0.7
    block = torch.full((T, 3), float("nan"), dtype=torch.float64, device=dev)  # column 0 of a projection, read in place
    block[:, 0] = torch.from_numpy(y).to(dev)
    for max_lag in sorted({0, T - 1, T + 3, 255, 256, 4096}):
        want, bound = tica.autocov_sums_host(y, max_lag), tc.autocov_bound(y, max_lag)
        for name, view in (("contiguous", torch.from_numpy(y).to(dev)), ("strided", block[:, 0])):
            big, out = guarded((max_lag + 1,), dev, torch.float64, SENTINEL)
            got = native.autocov_sums(view, max_lag, out=out)
            torch.cuda.synchronize()
            what = (T, max_lag, name)
            assert got.data_ptr() == out.data_ptr() and intact(big, SENTINEL), what
            g = got.cpu().numpy()
            assert (np.abs(g - want) <= 2 * bound).all(), what
            assert (g[T:] == 0).all() and (max_lag < 1 or T < 2 or g[: min(T, max_lag + 1)].any()), what
            assert np.array_equal(native.autocov_sums(view, max_lag).cpu().numpy(), g), what  # the same bits in every run
    # an infinite value is multiplied with the values it meets and with nothing behind the end
    z = y.copy()
    z[0] = np.inf
    g = native.autocov_sums(torch.from_numpy(z).to(dev), T + 3).cpu().numpy()
    w = tica.autocov_sums_host(z, T + 3)
    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w)) and (g[T:] == 0).all()


def test_the_c_entries_refuse_bad_arguments_and_write_nothing():
    import ctypes as C

    from jamun_amd import _lib, native

    dev = _dev()
    lib = _lib.load()
    T, W, lag, d, K = 70, 5, 3, 2, 9
    x = torch.from_numpy(np.array(tc.feature_rows(T, W))).to(dev)
    mean, v = torch.zeros(W, dtype=torch.float64, device=dev), torch.ones(W, d, dtype=torch.float64, device=dev)
    y = torch.ones(T, dtype=torch.float64, device=dev)
    need = C.c_int64(-1)
    assert lib.jamun_lagged_moments_work(T, W, lag, C.byref(need)) == 0 and need.value == 2 * W + 3 * W * W
    assert lib.jamun_lagged_moments_work(2 * SLICE + 4, 128, 3, C.byref(need)) == 0 and need.value == 3 * (2 * 128 + 3 * 128 * 128)
    assert lib.jamun_lagged_moments_work(0, W, lag, C.byref(need)) == 0 and need.value == 0
    assert lib.jamun_lagged_moments_work(T, W, T, C.byref(need)) == -1 and lib.jamun_lagged_moments_work(T, 129, 1, C.byref(need)) == -1
    assert lib.jamun_lagged_moments_work(T, W, lag, None) == -1 and b"null" in lib.jamun_last_error()
    assert lib.jamun_autocov_sums_work(T, K, C.byref(need)) == 0 and need.value == K + 1
    assert lib.jamun_autocov_sums_work(SLICE + 1, 4096, C.byref(need)) == 0 and need.value == 2 * 4097
    assert lib.jamun_autocov_sums_work(T, 4097, C.byref(need)) == -1 and lib.jamun_autocov_sums_work(-1, K, C.byref(need)) == -1
    big_s, sums = guarded((2, W), dev, torch.float64, SENTINEL)
    big_m, moments = guarded((3, W, W), dev, torch.float64, SENTINEL)
    big_w, work = guarded((2 * W + 3 * W * W,), dev, torch.float64, SENTINEL)
    big_p, proj = guarded((T, d), dev, torch.float64, SENTINEL)
    big_a, acf = guarded((K + 1,), dev, torch.float64, SENTINEL)
    big_k, awork = guarded((K + 1,), dev, torch.float64, SENTINEL)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda a: None if a is None else a.data_ptr()

    def mom(n_frames=T, width=W, lg=lag, stride=W, xs=x, s=sums, m=moments, w=work, cap=None):
        return lib.jamun_lagged_moments(p(xs), stride, n_frames, width, lg, p(s), p(m), p(w), work.numel() if cap is None else cap, st)

    def prj(n_frames=T, width=W, dd=d, stride=W, xs=x, mu=mean, vv=v, o=proj, cap=None):
        return lib.jamun_project_frames(p(xs), stride, n_frames, width, p(mu), p(vv), dd, p(o), proj.numel() if cap is None else cap, st)

    def acv(n_frames=T, max_lag=K, stride=1, ys=y, o=acf, w=awork, cap=None):
        return lib.jamun_autocov_sums(p(ys), stride, n_frames, max_lag, p(o), p(w), awork.numel() if cap is None else cap, st)

    err = lib.jamun_last_error
    assert mom(width=0) == -1 and mom(width=native.TICA_MAX_WIDTH + 1) == -1 and b"width" in err()
    assert mom(lg=0) == -1 and mom(lg=T) == -1 and b"lag" in err()
    assert mom(stride=W - 1) == -1 and b"row_stride" in err()
    assert mom(cap=work.numel() - 1) == -1 and b"work_capacity" in err()
    assert mom(n_frames=-1) == -1 and mom(cap=-1) == -1 and b"negative" in err()
    for null in ("xs", "s", "m", "w"):
        assert mom(**{null: None}) == -1 and b"null" in err(), null
    assert prj(width=0) == -1 and prj(width=129) == -1 and b"width" in err()
    assert prj(dd=0) == -1 and prj(dd=W + 1) == -1 and b"d " in err()
    assert prj(stride=W - 1) == -1 and b"row_stride" in err()
    assert prj(cap=T * d - 1) == -1 and b"out_capacity" in err()
    assert prj(n_frames=-1) == -1 and b"negative" in err()
    for null in ("xs", "mu", "vv", "o"):
        assert prj(**{null: None}) == -1 and b"null" in err(), null
    assert acv(max_lag=-1) == -1 and acv(max_lag=native.TICA_MAX_ACF_LAG + 1) == -1 and b"max_lag" in err()
    assert acv(stride=0) == -1 and b"stride" in err()
    assert acv(cap=K) == -1 and b"work_capacity" in err()
    assert acv(n_frames=-1) == -1 and acv(stride=-1) == -1 and b"negative" in err()
    for null in ("ys", "o", "w"):
        assert acv(**{null: None}) == -1 and b"null" in err(), null
    # no frames: nothing is launched, null pointers pass
    assert mom(n_frames=0) == 0 and mom(n_frames=0, xs=None, s=None, m=None, w=None, cap=0) == 0
    assert prj(n_frames=0) == 0 and prj(n_frames=0, xs=None, o=None, cap=0) == 0
    assert acv(n_frames=0) == 0 and acv(n_frames=0, ys=None, o=None, w=None, cap=0) == 0
    torch.cuda.synchronize()
    for big in (big_s, big_m, big_w, big_p, big_a, big_k):
        assert (big == SENTINEL).all()
    # and the same buffers take the results of good calls, the pads intact
    assert mom() == 0 and prj() == 0 and acv() == 0
    torch.cuda.synchronize()
    want_s, want_m = tica.lagged_moments_host(x.cpu().numpy(), lag)
    bound_s, bound_m = tc.moments_bounds(x.cpu().numpy(), lag)
    assert (np.abs(sums.cpu().numpy() - want_s) <= 2 * bound_s).all() and (np.abs(moments.cpu().numpy() - want_m) <= 2 * bound_m).all()
    want_p = tica.project_host(x.cpu().numpy(), mean.cpu().numpy(), v.cpu().numpy())  # (mean 0, weights 1: the row sums)
    assert (np.abs(proj.cpu().numpy() - want_p) <= 2 * tc.projection_bound(x.cpu().numpy(), mean.cpu().numpy(), v.cpu().numpy())).all()
    assert np.array_equal(acf.cpu().numpy(), np.arange(T, T - K - 1, -1.0))
    for big in (big_s, big_m, big_w, big_p, big_a, big_k):
        assert intact(big, SENTINEL)


# ---- the meter on the device path ----------------------------------------------------------------------------------------------------------------

def _kernel_features(meter, dev):
    """The meter's features from jamun_intcoord.hip whatever path the meter is on.  The device path's features are fp32 kernel values, the
    host path's the float64 formulas rounded to fp32: they differ in the last bits (test_gpu_intcoord.py holds that to its own bound), and
    with them everything behind them.  The comparison below is about jamun_tica.hip, so both runs start from the same feature rows."""
    from jamun_amd import native

    index = torch.from_numpy(meter.index).to(dev)

    def features(frames):
        frames = frames if torch.is_tensor(frames) else torch.from_numpy(np.asarray(frames))
        return native.internal_coords(frames.to(dev), index, cossin=True).cpu().numpy()

    return features


def test_meter_on_device_tensors_agrees_with_the_host_path_within_the_measured_tolerance(tmp_path):
    """Two batches of three chains of the dipeptide with driven torsions (`chain_view` blocks), 300 frames each, lag 5, and 1500 reference
    frames.  The tolerances are `_tica_cases.METER_TOLERANCE`: ten times what moving the reference moments by their rounding bound does to
    each output on this fixture, measured on the CPU (the JS distances did not move there: they are compared for equality)."""
    from jamun_amd.callbacks import TICAMetricsCallback

    dev = _dev()
    mol = dipeptide()
    ref, batches = tc.meter_fixture(mol, dev)
    assert all(s["xhat_traj"].transpose(0, 1).stride() == (3, 3 * tc.METER_CHAIN_T, 1) for b in batches for s in b)  # chain views, no copies
    kw = dict(lag=tc.METER_LAG, max_acf_lag=tc.METER_ACF_LAG)
    device_cb, device_smp = meter_run(TICAMetricsCallback, tmp_path / "device", mol, batches, dev, xyz=ref, device="device", **kw)

    class HostOnKernelFeatures(TICAMetricsCallback):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            for meter in self.meters.values():
                meter._features = _kernel_features(meter, dev)

    host_cb, host_smp = meter_run(HostOnKernelFeatures, tmp_path / "host", mol, batches, dev, xyz=ref, device="host", **kw)
    assert device_cb.meters["m"]._dev and not host_cb.meters["m"]._dev
    dd, hd = tmp_path / "device" / "m" / "tica", tmp_path / "host" / "m" / "tica"
    names = sorted(os.listdir(dd))
    assert names == sorted(os.listdir(hd)) == sorted([f"{i}.npz" for i in range(6)] + ["joined.npz", "model.json", "model.npz", "true_traj.npz"])
    assert open(dd / "model.json").read() == open(hd / "model.json").read()
    tol = tc.METER_TOLERANCE
    worst = {k: 0.0 for k in tol}
    a, b = np.load(dd / "model.npz"), np.load(hd / "model.npz")
    tc.check_gaps(b["eigenvalues"])
    for k in ("mean", "eigenvalues", "eigenvectors"):
        assert a[k].shape == b[k].shape
        worst[k] = float(np.abs(a[k] - b[k]).max())
    for name in names:
        if not name.endswith(".npz") or name == "model.npz":
            continue
        a, b = np.load(dd / name), np.load(hd / name)
        assert sorted(a.files) == sorted(b.files), name
        assert np.array_equal(a["num_frames"], b["num_frames"]) and a["tic01"].shape == b["tic01"].shape and np.isfinite(a["autocov"]).all(), name
        worst["tic01"] = max(worst["tic01"], float(np.abs(a["tic01"] - b["tic01"]).max()))
        worst["autocov"] = max(worst["autocov"], float(np.abs(a["autocov"] - b["autocov"]).max()))
        for k in ("js_distance_tic0", "js_distance_tic01"):
            if name != "true_traj.npz":
                worst["js_distance"] = max(worst["js_distance"], abs(float(a[k].item()) - float(b[k].item())))
    print("device path against host path, largest differences:", worst, "tolerances:", tol)
    for k in tol:
        assert worst[k] <= tol[k], (k, worst[k], tol[k])
    assert device_smp.fabric.logged == host_smp.fabric.logged and len(device_smp.fabric.logged) == 2


def test_device_mode_with_cpu_tensors_raises_the_meters_message(tmp_path):
    from jamun_amd.callbacks import TICAMetricsCallback

    dev = _dev()
    mol = dipeptide()
    ref, batches = tc.meter_fixture(mol, torch.device("cpu"))
    with pytest.raises(RuntimeError, match=r"TICAMetrics\(device='device'\) needs float32 sample tensors on a GPU"):
        meter_run(TICAMetricsCallback, tmp_path, mol, batches[:1], dev, xyz=ref, device="device", lag=tc.METER_LAG, max_acf_lag=tc.METER_ACF_LAG)
