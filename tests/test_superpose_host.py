"""CPU tests of the superposition: the host specification (`superpose.superpose_host`) against an independent fp64 reference, the premises
the GPU tests rest on (conditioning of the cases; a float32 model of the kernel's algorithm), ``SaveTrajectoryCallback(superpose=...)`` on
CPU tensors, and the argument checks of ``jamun_superpose_frames``."""
import os
import re

import numpy as np
import pytest
import torch

import _superpose_cases as sc
from _frames_common import CaseDataset, tree
from _traj_molecules import dipeptide

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RMSD_TOL_NM = sc.RMSD_TOL_NM


_case = sc.case  # (pos, frames, fp64 reference (aligned, rmsd, g)) of a molecule: computed once, shared, read only


# ------------------------------------------------------------------------------------------------------------ the host specification

@pytest.mark.parametrize("name", sc.COORD_MOLECULES)
def test_host_agrees_with_the_fp64_reference_in_every_frame(name):
    from jamun_amd.superpose import superpose_host

    pos, frames, (aligned, rmsd, g) = _case(name)
    got, got_rmsd = superpose_host(frames, pos)
    assert got.dtype == np.float32 and got_rmsd.dtype == np.float32 and got.shape == frames.shape and got_rmsd.shape == (frames.shape[0],)
    dev, dev_r = sc.frame_rmsd(got, aligned).max(), np.abs(got_rmsd - rmsd).max()
    print(f"{name}: host vs fp64 reference: coordinates {dev:.2e} nm, rmsd {dev_r:.2e} nm")
    assert dev <= RMSD_TOL_NM and dev_r <= RMSD_TOL_NM  # (fp64 both: what is left is the float32 rounding of the output, ~1e-7)


@pytest.mark.parametrize("name", sc.COORD_MOLECULES)
def test_host_returns_pos_for_a_rigid_image_and_not_for_the_mirror_image(name):
    from jamun_amd.superpose import superpose_host

    pos, frames, (aligned, rmsd, g) = _case(name)
    sl = sc.kind_slices(name)
    got, got_rmsd = superpose_host(frames, pos)
    for kind in ("identity", "turn180", "rigid"):
        assert sc.frame_rmsd(got[sl[kind]], np.broadcast_to(pos, got[sl[kind]].shape)).max() <= RMSD_TOL_NM, kind
        assert got_rmsd[sl[kind]].max() <= RMSD_TOL_NM, kind
    assert np.abs(got_rmsd[sl["mirror"]] - rmsd[sl["mirror"]]).max() <= RMSD_TOL_NM
    if name in sc.CHIRAL_MOLECULES:  # (a planar molecule's mirror image is a rotation away: _superpose_cases)
        assert rmsd[sl["mirror"]].min() > 100 * RMSD_TOL_NM  # the reference's rmsd: no proper rotation brings the mirror image back
        assert sc.frame_rmsd(got[sl["mirror"]], np.broadcast_to(pos, got[sl["mirror"]].shape)).min() > 100 * RMSD_TOL_NM
        # a rigid image all the same: a reflection would have shrunk the rmsd to 0, a proper rotation keeps the handedness of -pos
        assert np.abs(sc.pair_distances(got[sl["mirror"]]) - sc.pair_distances(pos[None])).max() <= 10 * RMSD_TOL_NM


@pytest.mark.parametrize("name", sc.RANK_DEFICIENT)
def test_host_on_rank_deficient_molecules_rmsd_and_shape_only(name):
    from jamun_amd.superpose import superpose_host

    pos, frames, (aligned, rmsd, g) = _case(name)
    assert g.max() <= 1e-6  # the premise of this list: no unique rotation
    got, got_rmsd = superpose_host(frames, pos)
    assert np.abs(got_rmsd - rmsd).max() <= RMSD_TOL_NM
    assert np.abs(sc.pair_distances(got) - sc.pair_distances(frames)).max() <= RMSD_TOL_NM  # a rigid image of the frame
    if pos.shape[0] == 1:
        assert np.array_equal(got, np.broadcast_to(pos, got.shape)) and not got_rmsd.any()


def test_host_non_finite_frame_stays_alone_and_arguments_are_checked():
    from jamun_amd.superpose import superpose, superpose_host

    pos, frames, _ = _case("dipeptide")
    clean, clean_rmsd = superpose_host(frames[:3], pos)
    poked = frames[:3].copy()
    poked[1, 4, 2] = np.nan
    got, got_rmsd = superpose_host(poked, pos)
    assert np.isnan(got[1]).all() and np.isnan(got_rmsd[1])
    assert np.array_equal(got[[0, 2]], clean[[0, 2]]) and np.array_equal(got_rmsd[[0, 2]], clean_rmsd[[0, 2]])
    with pytest.raises(ValueError):
        superpose_host(frames[:, :5], pos)
    # the public call on CPU data is the host path: arrays in, arrays out; tensors in, tensors out
    a, r = superpose(frames[:3], pos)
    assert isinstance(a, np.ndarray) and np.array_equal(a, clean) and np.array_equal(r, clean_rmsd)
    a, r = superpose(torch.from_numpy(frames[:3].copy()), torch.from_numpy(pos.copy()))
    assert torch.is_tensor(a) and np.array_equal(a.numpy(), clean) and np.array_equal(r.numpy(), clean_rmsd)


# ---------------------------------------------------------------------------------------------------------------------- the premises

def test_every_coordinate_case_is_well_conditioned():
    """Premise 1 of the coordinate comparisons (here and on the GPU): no frame of the coordinate cases sits near a degenerate rotation."""
    worst = {name: float(_case(name)[2][2].min()) for name in sc.COORD_MOLECULES}
    print("smallest eigenvalue gap g per molecule:", {k: round(v, 4) for k, v in worst.items()})
    assert min(worst.values()) >= sc.G_FLOOR, worst


def test_float32_model_of_the_kernel_stays_within_half_the_bound():
    """Premise 2: the kernel's ALGORITHM in float32 (numpy, one lane per frame: fp64 centroid sums, fp32 centred covariance, six cyclic
    Jacobi sweeps, the quaternion normalised by its norm, the RMSD from the aligned values) keeps half of RMSD_TOL_NM in reserve against
    the fp64 reference, in EVERY frame of the coordinate cases; the kernel may differ from the model by the order of a few roundings."""
    worst_c = worst_r = 0.0
    for name in sc.COORD_MOLECULES:
        pos, frames, (aligned, rmsd, g) = _case(name)
        got, got_rmsd = sc.kernel_model(frames, pos)
        assert got.dtype == np.float32 and got_rmsd.dtype == np.float32
        dc, dr = float(sc.frame_rmsd(got, aligned).max()), float(np.abs(got_rmsd.astype(np.float64) - rmsd).max())
        print(f"{name}: float32 model vs fp64 reference: coordinates {dc:.2e} nm, rmsd {dr:.2e} nm")
        worst_c, worst_r = max(worst_c, dc), max(worst_r, dr)
    print(f"largest: coordinates {worst_c:.2e} nm, rmsd {worst_r:.2e} nm")
    assert worst_c <= RMSD_TOL_NM / 2 and worst_r <= RMSD_TOL_NM / 2
    assert worst_c <= 1.5 * sc.MODEL_DEV_NM["coords"] and worst_r <= 1.5 * sc.MODEL_DEV_NM["rmsd"]  # (the recorded figures are current)


@pytest.mark.parametrize("name", sc.RANK_DEFICIENT)
def test_float32_model_on_rank_deficient_molecules(name):
    pos, frames, (aligned, rmsd, g) = _case(name)
    got, got_rmsd = sc.kernel_model(frames, pos)
    assert np.abs(got_rmsd - rmsd).max() <= RMSD_TOL_NM / 2
    assert np.abs(sc.pair_distances(got) - sc.pair_distances(frames)).max() <= RMSD_TOL_NM / 2
    if pos.shape[0] == 1:
        assert np.array_equal(got, np.broadcast_to(pos, got.shape)) and not got_rmsd.any()


# --------------------------------------------------------------------------------------------------------------------- the callback

def _batches(mol, chains=2, T=5, n_batches=2, seed=0):
    """Tumbling noisy images of the molecule as CPU samples [n, T, 3]."""
    rng = np.random.RandomState(seed)
    pos = mol["pos"].numpy().astype(np.float64)
    out = []
    for _ in range(n_batches):
        batch = []
        for _ in range(chains):
            rot = sc.random_rotations(rng, T)
            frames = np.einsum("fab,ib->fia", rot, pos) + rng.uniform(-0.5, 0.5, size=(T, 1, 3)) + sc.SIGMA * rng.randn(T, pos.shape[0], 3)
            batch.append({"dataset_label": "m", "xhat_traj": torch.from_numpy(np.ascontiguousarray(np.transpose(frames, (1, 0, 2)), dtype=np.float32))})
        out.append(batch)
    return out


def _run(cb, batches):
    smp = sc.CaseSampler(torch.device("cpu"))
    cb.on_sample_start(smp)
    for b in batches:
        cb.on_after_sample_batch(b, smp)
    cb.on_sample_end(smp)


def test_callback_superposes_pdb_and_dcd_keeps_npy_raw_and_writes_rmsd(tmp_path):
    from jamun_amd.callbacks import SaveTrajectoryCallback
    from jamun_amd.superpose import superpose_host

    mol = dipeptide()
    n, T = 10, 5
    batches = _batches(mol, chains=2, T=T, n_batches=2)
    ds = CaseDataset(mol, "m")
    _run(SaveTrajectoryCallback([ds], output_dir=str(tmp_path / "off")), batches)
    _run(SaveTrajectoryCallback([ds], output_dir=str(tmp_path / "on"), superpose=True), batches)
    off, on = tree(str(tmp_path / "off")), tree(str(tmp_path / "on"))
    rmsd_files = sorted(f for f in on if f.startswith(os.path.join("m", "predicted_samples", "rmsd")))
    assert rmsd_files == [os.path.join("m", "predicted_samples", "rmsd", f"{i}.npy") for i in (0, 1, 2, 3, "joined")]
    assert sorted(set(on) - set(rmsd_files)) == sorted(off)
    for f in off:  # .npy (and topology.pdb) identical to a run with the option off; .pdb / .dcd not
        assert (on[f] == off[f]) == (f.endswith(".npy") or f.endswith("topology.pdb")), f
    chains = [s["xhat_traj"].numpy() for b in batches for s in b]  # [n, T, 3] each, in the callback's order
    pred = tmp_path / "on" / "m" / "predicted_samples"
    names = [(str(i), np.transpose(c, (1, 0, 2))) for i, c in enumerate(chains)]
    names.append(("joined", np.concatenate([np.transpose(c, (1, 0, 2)) for c in chains])))  # spans both batches: 4 chains x 5 frames
    for name, raw in names:
        want, want_rmsd = superpose_host(raw, mol["pos"])
        assert want_rmsd.max() < 0.1 and sc.frame_rmsd(raw, np.broadcast_to(mol["pos"].numpy(), raw.shape)).min() > 0.1  # the fit did something
        assert np.array_equal(np.load(pred / "npy" / f"{name}.npy"), np.transpose(raw, (1, 0, 2)))
        got = sc.read_dcd_nm(str(pred / "dcd" / f"{name}.dcd"), n)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-6  # (x 10 and / 10 in float32: a relative 1e-7)
        assert np.abs(sc.read_pdb_milli_angstrom(str(pred / "pdb" / f"{name}.pdb"), n) - sc.milli_angstrom(want)).max() <= 1  # 1e-3 Angstrom
        got_rmsd = np.load(pred / "rmsd" / f"{name}.npy")
        assert got_rmsd.dtype == np.float32 and got_rmsd.shape == (raw.shape[0],) and np.abs(got_rmsd - want_rmsd).max() <= 1e-7
    assert np.load(pred / "rmsd" / "joined.npy").shape == (4 * T,)


def test_callback_superpose_needs_a_molecule_per_label():
    from jamun_amd.callbacks import SaveTrajectoryCallback

    class Bare:
        def label(self):
            return "bare"

    with pytest.raises(ValueError, match="bare"):
        SaveTrajectoryCallback([CaseDataset(dipeptide(), "m"), Bare()], superpose=True)
    SaveTrajectoryCallback([CaseDataset(dipeptide(), "m"), Bare()])  # off: as before


def test_callback_with_the_option_off_writes_what_it_wrote_without_the_argument(tmp_path):
    from jamun_amd.callbacks import SaveTrajectoryCallback

    mol = dipeptide()
    batches = _batches(mol, chains=2, T=4, n_batches=2, seed=1)
    ds = CaseDataset(mol, "m")
    _run(SaveTrajectoryCallback([ds], output_dir=str(tmp_path / "plain")), batches)
    _run(SaveTrajectoryCallback([ds], output_dir=str(tmp_path / "off"), superpose=False), batches)
    plain, off = tree(str(tmp_path / "plain")), tree(str(tmp_path / "off"))
    assert sorted(plain) == sorted(off) and plain == off
    assert not any("rmsd" in f for f in off) and len(off) == 1 + 3 * 5


def test_option_is_reachable_from_the_command_line(tmp_path):
    from jamun_amd import cmdline
    from jamun_amd import config as Cfg

    args = ["--config-dir=" + os.path.join(ROOT, "configs"), "experiment=sample_custom", "++init_pdbs=[a.pdb]", "++checkpoint_dir=ck"]
    on = Cfg.resolve(cmdline.compose(args + ["++callbacks.save_trajectory.superpose=true"], cwd=str(tmp_path)))
    assert on["callbacks"]["save_trajectory"]["superpose"] is True
    assert "superpose" not in Cfg.resolve(cmdline.compose(args, cwd=str(tmp_path)))["callbacks"]["save_trajectory"]  # the shipped yaml is as it was
    node = {k: v for k, v in on["callbacks"]["save_trajectory"].items() if k != "datasets"}  # (the datasets would be read from init_pdbs)
    cb = Cfg.instantiate(node, datasets=[CaseDataset(dipeptide(), "m")])
    assert cb.superpose is True


# -------------------------------------------------------------------------------------------------------------------------- the ABI

def test_symbol_is_declared_bound_and_exported():
    from jamun_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jamun_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    assert re.search(r"\bjamun_superpose_frames\s*\(", hdr)
    assert "jamun_superpose_frames" in _lib.SYMBOLS and hasattr(lib, "jamun_superpose_frames")
    assert len(_lib.SYMBOLS["jamun_superpose_frames"][1]) == 11
    assert lib.jamun_version() == 6  # additive: no struct changed
    from jamun_amd.csrc import build

    assert "jamun_superpose.hip" in build.SOURCES


def test_argument_errors_are_reported_without_a_gpu():
    from jamun_amd import _lib

    lib = _lib.load()
    INVALID = -1
    p, q = 1 << 20, 1 << 24  # (never dereferenced: every call below fails its argument checks before any device work)
    ok = dict(xyz=p, fs=3, as_=3 * 7, n=10, T=7, ref=p + 4096, out=q, ofs=3, oas=3 * 7, rmsd=q + 4096)

    def call(**over):
        a = dict(ok, **over)
        return lib.jamun_superpose_frames(a["xyz"], a["fs"], a["as_"], a["n"], a["T"], a["ref"], a["out"], a["ofs"], a["oas"], a["rmsd"], None)

    for null in ("xyz", "ref", "out"):
        assert call(**{null: None}) == INVALID and b"null" in lib.jamun_last_error(), null
    for neg in ("fs", "as_", "n", "T", "ofs", "oas"):
        assert call(**{neg: -1}) == INVALID and b"negative" in lib.jamun_last_error(), neg
    span = 4 * (6 * 3 + 9 * 21 + 3)  # bytes the input view spans
    # the output on top of the input with other strides; shifted by one frame; starting in the input's last float; ending in its first
    assert call(out=p, ofs=30, oas=3) == INVALID and b"overlaps" in lib.jamun_last_error()
    assert call(out=p + 12) == INVALID and b"overlaps" in lib.jamun_last_error()
    assert call(out=p + span - 4) == INVALID
    assert call(out=p - span + 4) == INVALID
    with pytest.raises(RuntimeError, match="jamun_hip error -1"):
        _lib.check(call(out=p + 12))
    # n_atoms and n_frames are int32 in the ABI: a count past 2^31 - 1 cannot be passed (it arrives wrapped, negative, and is refused)
    assert call(n=(1 << 31) + 5) == INVALID and call(T=(1 << 31) + 5) == INVALID
    # nothing to do is not an error, whatever the pointers overlap: no frame, or no atom
    assert call(T=0, out=p + 12) == 0 and call(n=0, out=p + 12) == 0
