"""GPU tests of the internal-coordinate kernel (jamun_intcoord.hip: k_internal_coords) and of ``SaveTrajectoryCallback(torsions=...)`` on the
device path.  Expected values are the numbers the analytic cases of _intcoord_cases.py were built from, and the fp64 host specification
on the molecule frames; the bounds TORSION_TOL_RAD / DIST_TOL_NM are the ones test_intcoord_host.py measures on a float32 model."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _intcoord_cases as ic
from _frames_common import CaseDataset, _dev, chain_view as _chain_view, guarded, intact, tree
from _traj_molecules import dipeptide

pytestmark = pytest.mark.gpu

TOL_A, TOL_D = ic.TORSION_TOL_RAD, ic.DIST_TOL_NM
SENTINEL = 12345.0  # 64 of them in front of and behind an output (`guarded`)


def _flat(frames: np.ndarray, dev) -> torch.Tensor:
    t = torch.from_numpy(np.array(frames, dtype=np.float32, order="C")).to(dev)
    assert t.is_contiguous()
    return t


def _check(got, want, index, cossin, what):
    ang, dist = ic.deviation(got, want, index, cossin)
    print(f"{what}: kernel vs expected: angles {ang:.2e} rad (bound {TOL_A:g}), distances {dist:.2e} nm (bound {TOL_D:g})")
    assert ang <= TOL_A and dist <= TOL_D, (what, ang, dist)


def _raw_call(frames: torch.Tensor, index: torch.Tensor, cossin: int, out: torch.Tensor, capacity=None) -> int:
    """The C entry itself, around the Python validation: returns its code."""
    from jamun_amd import _lib

    lib = _lib.load()
    with torch.cuda.device(frames.device):
        return lib.jamun_internal_coords(frames.data_ptr(), frames.stride(0), frames.stride(1), frames.shape[1], frames.shape[0], index.data_ptr(),
                                         index.shape[0], cossin, out.data_ptr(), out.numel() if capacity is None else capacity,
                                         torch.cuda.current_stream().cuda_stream)


# --------------------------------------------------------------------------------------------------- the kernel against the oracle

@pytest.mark.parametrize("cossin", [False, True], ids=["angles", "cossin"])
def test_analytic_cases_in_both_layouts(cossin):
    from jamun_amd import native

    dev = _dev()
    frames, expected = ic.analytic_case()
    frames = frames.astype(np.float32)
    want = ic.with_cossin(expected, ic.ANALYTIC_INDEX) if cossin else expected
    a = native.internal_coords(_chain_view(frames, dev), ic.ANALYTIC_INDEX, cossin=cossin)
    b = native.internal_coords(_flat(frames, dev), ic.ANALYTIC_INDEX, cossin=cossin)
    torch.cuda.synchronize()
    assert a.dtype == torch.float32 and tuple(a.shape) == want.shape and a.is_contiguous()
    assert torch.equal(a, b)
    _check(a.cpu().numpy(), want, ic.ANALYTIC_INDEX, cossin, f"analytic, cossin={int(cossin)}")
    got = a.cpu().numpy()
    if cossin:
        assert (got[:, 5] == 0).all()  # the constant beside a distance
    else:
        assert (got[:, 0] > -np.pi - 1e-6).all() and (got[:, 0] <= np.float32(np.pi)).all() and (got[:, 1] >= 0).all()


@pytest.mark.parametrize("cossin", [False, True], ids=["angles", "cossin"])
@pytest.mark.parametrize("name", ["dipeptide", "chain33"])
def test_molecule_frames_match_the_host_specification(name, cossin):
    from jamun_amd import native
    from jamun_amd.features import internal_coords_host

    dev = _dev()
    frames, index, _ = ic.molecule_case(name)
    got = native.internal_coords(_chain_view(frames, dev), index, cossin=cossin)
    _check(got.cpu().numpy(), internal_coords_host(frames, index, cossin=cossin), index, cossin, f"{name}, cossin={int(cossin)}")


FEATURE_TILE = 16  # IC_FTILE of jamun_intcoord.hip (test_intcoord_host.py checks that native.INTCOORD_FEATURE_TILE mirrors the kernel's)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
def test_frame_and_feature_counts_around_a_wave_and_a_tile(T):
    """A partial wave, exactly one, one frame over, several workgroups; 1, 2, 7 features and one less than, exactly and one more than a
    feature tile, distance, angle and dihedral rows interleaved: both layouts give the same bits, within the bounds of the fp64
    specification, inside a sentinel buffer whose floats in front and behind stay untouched."""
    from jamun_amd import native
    from jamun_amd.features import internal_coords_host

    dev = _dev()
    assert native.INTCOORD_FEATURE_TILE == FEATURE_TILE
    frames, pos = ic.rigid_case()
    frames = frames[:T]
    chain, flat = _chain_view(frames, dev), _flat(frames, dev)
    for F in (1, 2, 7, FEATURE_TILE - 1, FEATURE_TILE, FEATURE_TILE + 1):
        index = ic.mixed_table(pos, F, seed=F)
        assert sorted(set(ic.kinds(index).tolist())) == [2, 3, 4][: min(F, 3)]
        for cossin in (False, True):
            W = 2 * F if cossin else F
            big, out = guarded((T, W), dev, torch.float32, SENTINEL)
            got = native.internal_coords(chain, index, cossin=cossin, out=out)
            other = native.internal_coords(flat, index, cossin=cossin)
            torch.cuda.synchronize()
            assert got.data_ptr() == out.data_ptr() and torch.equal(got, other) and intact(big, SENTINEL)
            _check(got.cpu().numpy(), internal_coords_host(frames, index, cossin=cossin), index, cossin, f"T={T}, F={F}, cossin={int(cossin)}")


def test_empty_inputs_launch_nothing_and_succeed():
    from jamun_amd import native

    dev = _dev()
    frames, pos = ic.rigid_case()
    none = np.zeros((0, 4), dtype=np.int32)
    assert tuple(native.internal_coords(_flat(frames[:5], dev), none).shape) == (5, 0)
    assert tuple(native.internal_coords(_flat(frames[:0], dev), ic.mixed_table(pos, 3), cossin=True).shape) == (0, 6)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------ isolation

@pytest.mark.parametrize("cossin", [False, True], ids=["angles", "cossin"])
def test_non_finite_coordinates_spoil_exactly_their_features_in_their_frames(cossin):
    from jamun_amd import native

    dev = _dev()
    frames, index, _ = ic.molecule_case("chain33")
    frames = np.array(frames[:100])
    clean = native.internal_coords(_chain_view(frames, dev), index, cossin=cossin).cpu().numpy()
    poked = frames.copy()
    atom_a, atom_b = int(index[0, 1]), int(index[4, 0])
    poked[7, atom_a, 1] = np.nan
    poked[70, atom_b, 0] = np.inf
    got = native.internal_coords(_chain_view(poked, dev), index, cossin=cossin).cpu().numpy()
    m = 2 if cossin else 1
    bad = np.zeros(got.shape, dtype=bool)
    for t, atom in ((7, atom_a), (70, atom_b)):
        for j, (row, k) in enumerate(zip(index.tolist(), ic.kinds(index))):
            if atom in row[:k]:
                bad[t, m * j : m * j + m] = True
    assert bad.sum() >= 2 * m and np.isfinite(clean).all()
    assert not np.isfinite(got[bad]).any()
    assert np.array_equal(got[~bad].view(np.uint32), clean[~bad].view(np.uint32))  # bit for bit


@pytest.mark.parametrize("cossin", [0, 1], ids=["angles", "cossin"])
def test_a_row_with_an_index_out_of_range_is_nan_and_leaves_the_others_alone(cossin):
    """Straight to the C entry, around the Python validation: the kernel's own guard (the rule of jamun_edge_geometry) answers NaN and
    reads nothing; rows with fewer than two leading indices are NaN too."""
    dev = _dev()
    frames, pos = ic.rigid_case()
    chain = _chain_view(frames[:70], dev)
    good = ic.mixed_table(pos, 7, seed=7)
    table = good.copy()
    table[1] = [table[1][0], 33, table[1][2], -1]   # an angle whose middle atom is one past the last
    table[3] = [2 ** 31 - 1, 0, -1, -1]
    table[5] = [3, -1, 5, -1]                       # one leading index
    table[6] = [-1, -1, -1, -1]
    m = 2 if cossin else 1
    outs = []
    for t in (good, table):
        big, out = guarded((70, 7 * m), dev, torch.float32, SENTINEL)
        assert _raw_call(chain, torch.from_numpy(t).to(dev), cossin, out) == 0
        torch.cuda.synchronize()
        assert intact(big, SENTINEL)
        outs.append(out.cpu().numpy())
    clean, got = outs
    bad = np.zeros(got.shape, dtype=bool)
    for j in (1, 3, 5, 6):
        bad[:, m * j : m * j + m] = True
    assert np.isnan(got[bad]).all() and np.isfinite(clean).all()
    assert np.array_equal(got[~bad].view(np.uint32), clean[~bad].view(np.uint32))


def test_degenerate_geometry_gives_finite_output():
    from jamun_amd import native

    dev = _dev()
    p = np.zeros((2, 4, 3), dtype=np.float32)
    p[0, :, 0] = [0.0, 0.0, 0.15, 0.3]   # p0 == p1
    p[1, :, 0] = [0.0, 0.15, 0.3, 0.3]   # p0, p1, p2 on a line
    p[1, 3, 1] = 0.15
    table = np.array([[0, 1, 2, 3], [0, 1, 2, -1], [0, 1, -1, -1]], dtype=np.int32)
    for cossin in (False, True):
        assert torch.isfinite(native.internal_coords(_flat(p, dev), table, cossin=cossin)).all()


def test_out_capacity_too_small_is_invalid_and_writes_nothing():
    from jamun_amd import _lib

    dev = _dev()
    frames, pos = ic.rigid_case()
    chain = _chain_view(frames[:70], dev)
    index = torch.from_numpy(ic.mixed_table(pos, 7, seed=7)).to(dev)
    big, out = guarded((70, 14), dev, torch.float32, SENTINEL)
    assert _raw_call(chain, index, 1, out, capacity=70 * 14 - 1) == -1  # JAMUN_ERR_INVALID
    assert _raw_call(chain, index, 0, out, capacity=70 * 7 - 1) == -1
    assert b"out_capacity" in _lib.load().jamun_last_error()
    torch.cuda.synchronize()
    assert (big == SENTINEL).all()
    with pytest.raises(RuntimeError, match="out must be"):
        from jamun_amd import native

        native.internal_coords(chain, index, out=out[:, :7])  # (not contiguous)


def test_a_side_stream_call_is_ordered_behind_the_producer_of_its_input():
    from jamun_amd import native
    from jamun_amd.features import internal_coords_host

    dev = _dev()
    frames, pos = ic.rigid_case()
    index = ic.mixed_table(pos, 7, seed=7)
    half = torch.from_numpy(np.ascontiguousarray(np.transpose(frames, (1, 0, 2))) * np.float32(0.5)).to(dev)  # [n, T, 3]
    busy = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        for _ in range(8):
            busy = busy @ busy * 1e-3  # work in front of the producer, so that an unordered kernel would read the input too early
        chain = half + half            # exact: the frames, produced on the side stream
        got = native.internal_coords(chain.transpose(0, 1), index)
    side.synchronize()
    _check(got.cpu().numpy(), internal_coords_host(frames, index), index, False, "side stream")


def test_public_call_takes_the_kernel_for_device_tensors():
    from jamun_amd import native
    from jamun_amd.features import internal_coords

    dev = _dev()
    frames, index, _ = ic.molecule_case("dipeptide")
    x = _flat(frames, dev)
    a = internal_coords(x, index, cossin=True)
    assert a.is_cuda and a.dtype == torch.float32 and torch.equal(a, native.internal_coords(x, index, cossin=True))
    on_dev = torch.from_numpy(np.array(index)).to(dev)
    assert torch.equal(native.internal_coords(x, on_dev, cossin=True), a)  # a table uploaded once
    with pytest.raises(ValueError, match="index table"):
        native.internal_coords(x, on_dev.to(torch.int64))


# ------------------------------------------------------------------------------------------------- the callback on the device path

@pytest.mark.parametrize("staging", [None, 1 << 12, 1 << 8], ids=["staging_default", "staging_4k", "staging_256"])
def test_callback_device_path_writes_the_host_path_torsions(tmp_path, monkeypatch, staging):
    """3 chains of the dipeptide x 70 frames, two batches, torsions="all".  With 4 KiB of staging the .pdb / .dcd encoders take a chain in
    several chunks; with 256 bytes the torsions do too (21 frames of 3 angles per chunk; a PDB model no longer fits: the host formatter)."""
    from jamun_amd import traj_encode
    from jamun_amd.callbacks import SaveTrajectoryCallback

    if staging is not None:
        monkeypatch.setattr(traj_encode, "STAGING_BYTES", staging)
    dev = _dev()
    mol = dipeptide()
    n, T, chains = 10, 70, 3
    batches = ic.tumbling_batches(mol, dev, chains, T, 2, seed=5, sigma=0.01)
    ds = CaseDataset(mol, "m")
    cbs = {m: ic.run_callback(SaveTrajectoryCallback([ds], output_dir=str(tmp_path / m), encode=m, torsions="all"), batches, dev) for m in ("device", "host")}
    raw = ic.run_callback(SaveTrajectoryCallback([ds], output_dir=str(tmp_path / "raw"), encode="device"), batches, dev)
    assert cbs["device"]._encoder is not None and cbs["host"]._encoder is None
    assert not cbs["device"]._dev_blocks and not raw._dev_blocks
    assert cbs["device"]._encoder.staging_bytes() == raw._encoder.staging_bytes() == 3 * traj_encode.STAGING_BYTES
    trees = {m: tree(str(tmp_path / m)) for m in ("device", "host", "raw")}
    assert sorted(trees["device"]) == sorted(trees["host"])
    tors = sorted(f for f in trees["device"] if "torsion" in f)
    assert len(tors) == 2 * chains + 2
    assert {f: d for f, d in trees["device"].items() if "torsion" not in f} == trees["raw"]  # byte for byte the run without the option
    assert trees["device"][os.path.join("m", "torsion_labels.json")] == trees["host"][os.path.join("m", "torsion_labels.json")]
    index = cbs["device"]._states["m"].tor_index
    assert index.shape == (3, 4)
    d, h = (tmp_path / m / "m" / "predicted_samples" / "torsions" for m in ("device", "host"))
    for name in [str(i) for i in range(2 * chains)] + ["joined"]:
        got, want = np.load(d / f"{name}.npy"), np.load(h / f"{name}.npy")
        assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == ((2 * chains * T if name == "joined" else T), 3)
        dev_t = float(np.abs(ic.wrapped(got, want)).max())
        print(f"{name}: device vs host torsion files: {dev_t:.2e} rad")
        assert dev_t <= TOL_A
    assert np.array_equal(np.load(d / "joined.npy"), np.concatenate([np.load(d / f"{i}.npy") for i in range(2 * chains)]))
    for b in batches:  # the premise of the comparison: the frames are conditioned as the molecule cases are
        for s in b:
            assert ic._well_conditioned(s["xhat_traj"].permute(1, 0, 2).double().cpu().numpy(), index).all()
