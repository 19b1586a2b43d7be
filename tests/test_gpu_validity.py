"""GPU tests of jamun_validity.hip (k_validity_frames) and of the chemical-validity meter on the device path.  The expected values are the
host specification's (jamun_amd/validity.py: `validity_counts_host`, itself pinned in test_validity_host.py to a per-pair sqrt-and-compare
loop and to the reference's recorded results): every count is an integer and must be EQUAL, nothing is compared within a tolerance."""
import os

import numpy as np
import pytest
import torch

import _validity_cases as vc
from _frames_common import _dev, guarded, intact, meter_run, tree
from _traj_molecules import dipeptide
from jamun_amd import validity as V

pytestmark = pytest.mark.gpu

SENTINEL = -77
CHUNK, SPLIT, MAX_ATOMS = 64, 32, 256  # the seams of the kernel as built (test_validity_host.py checks that native mirrors the header)
T_MAX = 129


def _layouts(frames3: np.ndarray, T: int, dev):
    """``frames3 [3 T_MAX, n, 3]`` -> (name, device view [T, n, 3], the same frames on the host) for the three layouts."""
    n = frames3.shape[1]
    first = np.array(frames3[:T])  # (copies: the cached frames are read only)
    block = torch.from_numpy(np.array(first.transpose(1, 0, 2), order="C")).to(dev)  # [n, T, 3], as a chain is kept
    yield "chain", block.transpose(0, 1), first
    yield "contiguous", torch.from_numpy(first).to(dev), first
    wide = torch.from_numpy(np.array(frames3[: 3 * T].transpose(1, 0, 2), order="C")).to(dev)  # [n, 3 T, 3]
    view = wide.transpose(0, 1)[::3]
    assert tuple(view.shape) == (T, n, 3) and (T == 1 or view.stride(0) == 9)
    yield "every third", view, np.array(frames3[: 3 * T : 3])


def _u32(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n", [1, 2, 3, 17, SPLIT - 1, SPLIT, SPLIT + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, MAX_ATOMS])
def test_counts_and_bond_frames_equal_the_host_specification_integer_for_integer(n):
    """Frame counts around a wave; atom counts at 1, 2, 3, 17, either side of the wave split and of one and two LDS chunks, and the
    limit; no bond, a tree and every pair bonded; a chain view, a contiguous block and every third frame of a chain; outputs inside
    sentinel-guarded buffers."""
    from jamun_amd import native

    dev = _dev()
    assert (native.VALIDITY_CHUNK, native.VALIDITY_SPLIT_ATOMS, native.VALIDITY_MAX_ATOMS) == (CHUNK, SPLIT, MAX_ATOMS)
    frames3 = vc.helix_frames(n, 3 * T_MAX)
    seen = np.zeros(2, dtype=np.int64)
    for kind in ("none", "tree", "all"):
        tables = V.validity_tables(vc.helix(n, kind), *vc.HELIX_TOLERANCES)
        on_dev = native.upload_validity_tables(tables, n, dev)
        B = tables["num_bonds"]
        for T in (1, 63, 64, 65, T_MAX):
            for name, view, host in _layouts(frames3, T, dev):
                want, want_bf = V.validity_counts_host(host, tables)
                big, out = guarded((T, 2), dev, torch.int32, SENTINEL)
                big_b, bf = guarded((B,), dev, torch.int32, SENTINEL)
                got, got_bf = native.validity_counts(view, on_dev, out=out, bond_frames=bf)
                torch.cuda.synchronize()
                what = (n, kind, T, name)
                assert got.data_ptr() == out.data_ptr() and got_bf.data_ptr() == bf.data_ptr() and intact(big, SENTINEL) and intact(big_b, SENTINEL), what
                assert np.array_equal(_u32(got), want), what
                assert np.array_equal(_u32(got_bf), want_bf), what
                seen += want.sum(axis=0).astype(np.int64)
        if kind == "tree" and n >= 3:
            vc.check_varied(want)  # (T_MAX frames, every third: each count zero in some frames, non-zero in others)
    assert n < 2 or seen[1] > 0
    assert n < 3 or seen[0] > 0


def _two_atoms(dev):
    x = np.array([[[0.125, -0.25, 0.5], [0.25, -0.125, 0.375]]], dtype=np.float32)  # [1, 2, 3]
    d = x[0, 1] - x[0, 0]
    s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    assert s.dtype == np.float32 and s > 0
    return torch.from_numpy(x).to(dev), s


def test_the_comparisons_are_strict():
    """Hand-made tables S = s and the float32 either side of it, for the s of a two-atom frame: a clash only for s < S; a bond issue only
    for s > S_hi or s < S_lo."""
    from jamun_amd import native

    dev = _dev()
    x, s = _two_atoms(dev)
    below, above = np.nextafter(s, np.float32(-np.inf)), np.nextafter(s, np.float32(np.inf))
    f = lambda *v: np.array(v, dtype=np.float32)
    none = {"bonds": np.zeros((0, 2), dtype=np.int32), "bond_lo_s": f(), "bond_hi_s": f()}
    for S, clash in ((below, 0), (s, 0), (above, 1)):
        got, _ = native.validity_counts(x, dict(none, clash_s=f(S)))
        assert _u32(got).tolist() == [[clash, 0]], (S, clash)
    bond = {"clash_s": f(0.0), "bonds": np.array([[0, 1]], dtype=np.int32)}
    zero, inf = np.float32(0.0), np.float32(np.inf)
    for lo, hi, off in ((zero, below, 1), (zero, s, 0), (zero, above, 0), (below, inf, 0), (s, inf, 0), (above, inf, 1), (above, below, 1)):
        got, bf = native.validity_counts(x, dict(bond, bond_lo_s=f(lo), bond_hi_s=f(hi)))
        assert _u32(got).tolist() == [[0, off]] and _u32(bf).tolist() == [off], (lo, hi, off)


@pytest.mark.parametrize("n", [17, CHUNK + 1])
def test_a_non_finite_coordinate_changes_its_own_frame_as_the_host_says_and_no_other(n):
    from jamun_amd import native

    dev = _dev()
    tables = V.validity_tables(vc.helix(n), *vc.HELIX_TOLERANCES)
    clean = np.array(vc.helix_frames(n, T_MAX))
    want_clean, _ = V.validity_counts_host(clean, tables)
    got_clean, _ = native.validity_counts(torch.from_numpy(clean).to(dev), tables)
    assert np.array_equal(_u32(got_clean), want_clean)
    changed = 0
    for value in (np.nan, np.inf, -np.inf):
        for t, a, c in ((0, 0, 0), (64, n - 1, 2), (T_MAX - 1, n // 2, 1)):
            x = clean.copy()
            x[t, a, c] = value
            want, want_bf = V.validity_counts_host(x, tables)
            got, got_bf = native.validity_counts(torch.from_numpy(x).to(dev).transpose(0, 1).contiguous().transpose(0, 1), tables)
            got = _u32(got)
            assert np.array_equal(got, want) and np.array_equal(_u32(got_bf), want_bf), (value, t, a)
            others = np.arange(T_MAX) != t
            assert np.array_equal(got[others], want_clean[others]), (value, t, a)
            if np.isinf(value):  # every bond of the atom has s = inf: off; (a NaN compares false: no issue)
                assert got[t, 1] >= 1
            changed += int((got[t] != want_clean[t]).any())
    assert changed > 0


def test_the_c_entry_refuses_bad_arguments_and_writes_nothing():
    from jamun_amd import _lib, native

    dev = _dev()
    lib = _lib.load()
    n, T = 5, 70
    tables = V.validity_tables(vc.helix(n), *vc.HELIX_TOLERANCES)
    t = native.upload_validity_tables(tables, n, dev)
    B = tables["num_bonds"]
    x = torch.from_numpy(np.array(vc.helix_frames(n, T))).to(dev)
    big, out = guarded((T, 2), dev, torch.int32, SENTINEL)
    big_b, bf = guarded((B,), dev, torch.int32, SENTINEL)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda a: None if a is None else a.data_ptr()

    def call(n_atoms=n, n_frames=T, capacity=None, n_bonds=B, xyz=x, clash=t["clash_s"], bonds=t["bonds"], lo=t["bond_lo_s"], hi=t["bond_hi_s"],
             counts=out, frames_of_bond=bf):
        return lib.jamun_validity_counts(p(xyz), 3 * n, 3, n_atoms, n_frames, p(clash), p(bonds), p(lo), p(hi), n_bonds, p(counts),
                                         2 * T if capacity is None else capacity, p(frames_of_bond), st)

    assert call(n_atoms=native.VALIDITY_MAX_ATOMS + 1) == -1 and b"n_atoms" in lib.jamun_last_error()
    assert call(n_atoms=0) == -1 and b"n_atoms" in lib.jamun_last_error()
    assert call(capacity=2 * T - 1) == -1 and b"counts_capacity" in lib.jamun_last_error()
    assert call(n_frames=-1) == -1 and call(n_bonds=-1) == -1 and b"negative" in lib.jamun_last_error()
    for null in ("xyz", "clash", "bonds", "lo", "hi", "counts"):
        assert call(**{null: None}) == -1 and b"null" in lib.jamun_last_error(), null
    torch.cuda.synchronize()
    assert (big == SENTINEL).all() and (big_b == SENTINEL).all()
    assert call(n_frames=0) == 0 and call(n_frames=0, xyz=None, counts=None, capacity=0) == 0
    torch.cuda.synchronize()
    assert (big == SENTINEL).all() and (big_b == SENTINEL).all()
    want, want_bf = V.validity_counts_host(x.cpu().numpy(), tables)
    assert call(frames_of_bond=None) == 0  # (no per-bond counts asked for)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(out), want) and (big_b == SENTINEL).all() and intact(big, SENTINEL)
    assert call(n_bonds=0, bonds=None, lo=None, hi=None, frames_of_bond=None) == 0  # (no bonds: NULL bond pointers)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(out)[:, 0], want[:, 0]) and not _u32(out)[:, 1].any()
    assert call(n_atoms=1, clash=None, n_bonds=0, bonds=None, lo=None, hi=None) == 0  # (one atom: zeros)
    torch.cuda.synchronize()
    assert not _u32(out).any() and intact(big, SENTINEL)
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(_u32(out), want) and np.array_equal(_u32(bf), want_bf) and intact(big, SENTINEL) and intact(big_b, SENTINEL)
    # the wrapper checks a host bond table before anything is uploaded
    for bad in ([[0, n]], [[-1, 0]], [[2, 2]]):
        with pytest.raises(ValueError, match="bond 0"):
            native.validity_counts(x, dict(tables, bonds=np.array(bad, dtype=np.int32), bond_lo_s=tables["bond_lo_s"][:1], bond_hi_s=tables["bond_hi_s"][:1]))
    # ... and the kernel skips a bond out of range in a table that is already on the device
    raw = dict(t, bonds=torch.tensor([[0, 1], [0, n], [-1, 2], [1, 2]], dtype=torch.int32, device=dev), bond_lo_s=t["bond_lo_s"][[0, 0, 0, 1]].contiguous(),
               bond_hi_s=t["bond_hi_s"][[0, 0, 0, 1]].contiguous())
    got, got_bf = native.validity_counts(x, raw)
    two = V.validity_counts_host(x.cpu().numpy(), dict(tables, bonds=tables["bonds"][:2], bond_lo_s=tables["bond_lo_s"][:2], bond_hi_s=tables["bond_hi_s"][:2]))
    assert np.array_equal(_u32(got)[:, 1], two[0][:, 1]) and _u32(got_bf)[[0, 3]].tolist() == two[1].tolist() and not _u32(got_bf)[[1, 2]].any()


@pytest.mark.parametrize("n", [17, CHUNK + 1])
def test_a_second_call_gives_the_same_bits_whatever_the_buffers_held(n):
    from jamun_amd import native

    dev = _dev()
    tables = V.validity_tables(vc.helix(n), *vc.HELIX_TOLERANCES)
    x = torch.from_numpy(np.array(vc.helix_frames(n, T_MAX))).to(dev)
    first, first_bf = native.validity_counts(x, tables)
    out = torch.full((T_MAX, 2), 123456789, dtype=torch.int32, device=dev)
    bf = torch.full((tables["num_bonds"],), -5, dtype=torch.int32, device=dev)
    native.validity_counts(x, tables, out=out, bond_frames=bf)
    assert torch.equal(first, out) and torch.equal(first_bf, bf) and int(first.sum()) > 0
    native.validity_counts(x, tables, out=out, bond_frames=bf)  # (again into the results themselves: nothing accumulates)
    assert torch.equal(first, out) and torch.equal(first_bf, bf)


# ---- the meter on the device path --------------------------------------------------------------------------------------------------------

def _meter_run(root, mol, batches, dev, xyz=None, **kw):
    from jamun_amd.callbacks import ChemicalValidityMetricsCallback

    vtol, btol = kw.pop("tolerances")
    return meter_run(ChemicalValidityMetricsCallback, root, mol, batches, dev, xyz=xyz, volume_exclusion_tolerance=vtol, bond_length_tolerance=btol, **kw)


@pytest.mark.parametrize("num", [100, None])
def test_meter_on_device_tensors_writes_the_host_paths_files_byte_for_byte(tmp_path, num):
    """Two batches of three chains of the dipeptide, 350 frames each (every third frame at 100 per trajectory: all four noise levels), and 300
    frames of its own as the dataset's trajectory."""
    dev = _dev()
    mol = dipeptide()
    batches = vc.chain_batches(mol, dev, 3, 350, 2, seed=40)
    xyz = torch.from_numpy(np.array(vc.dipeptide_frames(300)))
    runs = {mode: _meter_run(tmp_path / mode, mol, batches, dev, xyz=xyz, tolerances=vc.DIPEPTIDE_TOLERANCES, num_molecules_per_trajectory=num,
                             device=mode) for mode in ("device", "host")}
    d, h = tree(str(tmp_path / "device")), tree(str(tmp_path / "host"))
    base = os.path.join("m", "chemical_validity")
    assert sorted(d) == sorted(os.path.join(base, f) for f in [f"{i}.npz" for i in range(6)] + ["joined.npz", "tables.json", "true_traj.npz"])
    assert d == h
    assert runs["device"][1].fabric.logged == runs["host"][1].fabric.logged and len(runs["device"][1].fabric.logged) == 2
    assert runs["device"][0].meters["m"]._dev and not runs["host"][0].meters["m"]._dev
    z = np.load(tmp_path / "device" / base / "joined.npz")
    K = 350 if num is None else 117  # (350 // 100 = 3: every third frame)
    assert z["frame_indices"].shape == (6 * K,) and z["frame_indices"][K] == 350
    vc.check_varied(np.stack([z["clash_counts"], z["bond_counts"]], axis=1))


def test_a_molecule_above_the_limit_takes_the_host_path_under_auto_and_raises_under_device(tmp_path):
    from jamun_amd import native

    dev = _dev()
    mol = vc.helix(native.VALIDITY_MAX_ATOMS + 1)
    batches = vc.chain_batches(mol, dev, 1, 20, 1, seed=50)
    auto, _ = _meter_run(tmp_path / "auto", mol, batches, dev, tolerances=vc.HELIX_TOLERANCES, device="auto")
    _meter_run(tmp_path / "host", mol, batches, dev, tolerances=vc.HELIX_TOLERANCES, device="host")
    assert not auto.meters["m"]._dev and tree(str(tmp_path / "auto")) == tree(str(tmp_path / "host"))
    with pytest.raises(RuntimeError, match="at most 256 atoms"):
        _meter_run(tmp_path / "device", mol, batches, dev, tolerances=vc.HELIX_TOLERANCES, device="device")
