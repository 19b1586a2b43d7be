"""CPU tests of the internal coordinates: the fp64 host specification against analytic geometry, the MEASURED tolerances of the GPU tests,
the torsion and C-alpha tables, the index-table validation of ``native.internal_coords`` and ``SaveTrajectoryCallback(torsions=...)`` on
the host path.  (test_gpu_intcoord.py holds the kernel to the same cases.)"""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import _intcoord_cases as ic
from _frames_common import CaseDataset, tree
from _traj_molecules import dipeptide

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mol(names, residues, seq, chain=None, seed=0):
    n = len(names)
    mol = dict(pos=torch.from_numpy(np.random.RandomState(seed).randn(n, 3).astype(np.float32) * 0.3), atom_names=list(names), residues=list(residues),
               residue_sequence_index=torch.tensor(seq, dtype=torch.int32), atom_type_index=torch.zeros(n, dtype=torch.int32),
               elements=[a[0] for a in names], residue_ids=[int(i) + 1 for i in seq], bonds=torch.zeros((2, 0), dtype=torch.long))
    if chain is not None:
        mol["chain_index"] = list(chain)
    return mol


def ace_ala_nme():
    names = ["CH3", "C", "O", "N", "CA", "CB", "C", "O", "N", "CH3"]
    return _mol(names, ["ACE"] * 3 + ["ALA"] * 5 + ["NME"] * 2, [0] * 3 + [1] * 5 + [2] * 2)


def pro_ala():
    """Two free residues; the first carries a side chain with CG and CD and nothing beyond."""
    names = ["N", "CA", "CB", "CG", "CD", "C", "O", "N", "CA", "CB", "C", "O", "OXT"]
    return _mol(names, ["PRO"] * 7 + ["ALA"] * 6, [0] * 7 + [1] * 6)


# ------------------------------------------------------------------------------------------------------------ the host specification

def test_host_specification_reproduces_the_analytic_values():
    from jamun_amd.features import internal_coords_host

    frames, expected = ic.analytic_case()
    got = internal_coords_host(frames, ic.ANALYTIC_INDEX)
    assert got.dtype == np.float64 and got.shape == expected.shape
    ang, dist = ic.deviation(got, expected, ic.ANALYTIC_INDEX)
    pair = internal_coords_host(frames, ic.ANALYTIC_INDEX, cossin=True)
    ang_cs, dist_cs = ic.deviation(pair, ic.with_cossin(expected, ic.ANALYTIC_INDEX), ic.ANALYTIC_INDEX, cossin=True)
    print(f"fp64 specification vs analytic: angles {ang:.2e} rad, distances {dist:.2e} nm; cos / sin {ang_cs:.2e}, (d, 0) {dist_cs:.2e}")
    assert max(ang, dist, ang_cs, dist_cs) <= 1e-12
    assert (got[:, 0] > -math.pi).all() and (got[:, 0] <= math.pi).all() and (got[:, 1] >= 0).all() and (got[:, 1] <= math.pi).all()
    assert (pair[:, 5] == 0).all()  # the constant beside a distance


def test_host_specification_nan_rules_and_degenerate_geometry():
    from jamun_amd.features import internal_coords_host

    frames = np.array(ic.analytic_case()[0][:6])
    table = np.array([[0, 1, 2, 3], [3, -1, 5, -1], [0, 9, -1, -1], [-1, -1, -1, -1], [4, 5, 6, -1], [7, 8, -1, -1]])
    frames[2, 5, 1] = np.inf  # atom 5 is in the angle row only
    frames[4, 0, 0] = np.nan  # atom 0 is in the dihedral row only
    for cossin in (False, True):
        got = internal_coords_host(frames, table, cossin=cossin)
        m = 2 if cossin else 1
        bad = np.zeros(got.shape, dtype=bool)
        bad[:, m * 1 : m * 4] = True  # one leading index, an index >= n, no index
        bad[2, m * 4 : m * 5] = True
        bad[4, 0:m] = True
        assert np.array_equal(np.isnan(got), bad) and np.isfinite(got[~bad]).all()
    # coincident atoms and a collinear triple inside a dihedral: finite, whatever atan2 says
    p = np.zeros((2, 4, 3))
    p[0, :, 0] = [0.0, 0.0, 0.15, 0.3]          # p0 == p1
    p[1, :, 0] = [0.0, 0.15, 0.3, 0.3]          # p0, p1, p2 on a line
    p[1, 3, 1] = 0.15
    for cossin in (False, True):
        assert np.isfinite(internal_coords_host(p, np.array([[0, 1, 2, 3], [0, 1, 2, -1], [0, 1, -1, -1]]), cossin=cossin)).all()
    assert internal_coords_host(p, np.zeros((0, 4), dtype=np.int32)).shape == (2, 0)


def test_public_call_takes_the_host_path_for_cpu_inputs():
    from jamun_amd.features import internal_coords, internal_coords_host

    frames, _ = ic.analytic_case()
    want = internal_coords_host(frames, ic.ANALYTIC_INDEX, cossin=True)
    assert np.array_equal(internal_coords(frames, ic.ANALYTIC_INDEX, cossin=True), want)
    got = internal_coords(torch.from_numpy(np.array(frames)), ic.ANALYTIC_INDEX, cossin=True)
    assert torch.is_tensor(got) and np.array_equal(got.numpy(), want)


# ------------------------------------------------------------------------------------------------------------- the measured tolerances

def _round_up_one_digit(v: float) -> float:
    e = math.floor(math.log10(v))
    return float(f"{math.ceil(v / 10 ** e - 1e-9)}e{e}")


def test_molecule_cases_drop_at_most_five_percent_of_the_drawn_frames():
    for name in ("dipeptide", "chain33"):
        frames, index, dropped = ic.molecule_case(name)
        print(f"{name}: {frames.shape[0]} of {ic.N_MOLECULE_FRAMES} frames kept, {100 * dropped:.2f} % dropped; {index.shape[0]} features")
        assert dropped <= 0.05 and frames.shape[0] >= 0.95 * ic.N_MOLECULE_FRAMES
    assert ic.molecule_case("chain33")[1].shape[0] > 16  # (more than one feature tile of the kernel)


def test_tolerances_are_four_times_the_float32_models_deviation():
    """TORSION_TOL_RAD / DIST_TOL_NM are measured, not chosen: a float32 numpy model of the kernel's arithmetic over every case of
    _intcoord_cases.py, against the analytic values (which the GPU test compares with: this includes the rounding of the frames to
    float32) and against the fp64 specification on the same float32 frames; four times the worst, rounded up to one digit (the factor
    covers atan2f against numpy's arctan2 and a different summation order).  1e-4 rad is 1/600 of a bin of the reference's 100-bin
    Ramachandran histogram, the coarsest thing these angles feed."""
    from jamun_amd.features import internal_coords_host

    frames, expected = ic.analytic_case()
    f32 = frames.astype(np.float32)
    ang_worst = dist_worst = 0.0
    for cossin in (False, True):
        model = ic.kernel_model(f32, ic.ANALYTIC_INDEX, cossin)
        want = ic.with_cossin(expected, ic.ANALYTIC_INDEX) if cossin else expected
        cases = [("analytic", model, want, ic.ANALYTIC_INDEX), ("analytic frames vs fp64", model, internal_coords_host(f32, ic.ANALYTIC_INDEX, cossin), ic.ANALYTIC_INDEX)]
        for name in ("dipeptide", "chain33"):
            mf, index, _ = ic.molecule_case(name)
            cases.append((name + " vs fp64", ic.kernel_model(mf, index, cossin), internal_coords_host(mf, index, cossin), index))
        rigid, pos = ic.rigid_case()
        for F in (1, 2, 7, 15, 16, 17):
            index = ic.mixed_table(pos, F, seed=F)
            cases.append((f"rigid chain33, {F} features, vs fp64", ic.kernel_model(rigid, index, cossin), internal_coords_host(rigid, index, cossin), index))
        for what, got, ref, index in cases:
            ang, dist = ic.deviation(got, ref, index, cossin)
            print(f"float32 model, cossin={int(cossin)}, {what}: angles {ang:.3e} rad, distances {dist:.3e} nm")
            ang_worst, dist_worst = max(ang_worst, ang), max(dist_worst, dist)
    tol_a, tol_d = _round_up_one_digit(4 * ang_worst), _round_up_one_digit(4 * dist_worst)
    print(f"worst: {ang_worst:.3e} rad, {dist_worst:.3e} nm -> TORSION_TOL_RAD {tol_a:g}, DIST_TOL_NM {tol_d:g}")
    assert tol_a == ic.TORSION_TOL_RAD and tol_d == ic.DIST_TOL_NM
    assert ic.TORSION_TOL_RAD <= 1e-4 and ic.DIST_TOL_NM <= 1e-6


# ------------------------------------------------------------------------------------------------------------------ which atoms

def test_torsion_indices_of_the_capped_alanine():
    from jamun_amd.features import torsion_indices

    mol = ace_ala_nme()
    index, labels = torsion_indices(mol)
    assert index.dtype == np.int32 and index.shape == (2, 4)
    assert labels == ["PHI 0 ALA 1", "PSI 0 ALA 1"]  # one phi, one psi, no omega
    names = [[mol["atom_names"][i] for i in row] for row in index]
    assert names == [["C", "N", "CA", "C"], ["N", "CA", "C", "N"]]
    assert index.tolist() == [[1, 3, 4, 6], [3, 4, 6, 8]]
    assert torsion_indices(mol, sidechain=True)[1] == labels  # (CB and nothing beyond: no chi)
    assert torsion_indices(mol, backbone=False)[0].shape == (0, 4)


def test_torsion_indices_of_two_free_residues_with_a_side_chain():
    from jamun_amd.features import torsion_indices

    mol = pro_ala()
    index, labels = torsion_indices(mol, sidechain=True)
    assert labels == ["PHI 0 ALA 1", "PSI 0 PRO 0", "OMEGA 0 PRO 0", "CHI1 0 PRO 0", "CHI2 0 PRO 0"]
    assert [[mol["atom_names"][i] for i in row] for row in index] == [["C", "N", "CA", "C"], ["N", "CA", "C", "N"], ["CA", "C", "N", "CA"],
                                                                      ["N", "CA", "CB", "CG"], ["CA", "CB", "CG", "CD"]]
    assert index.tolist() == [[5, 7, 8, 10], [0, 1, 5, 7], [1, 5, 7, 8], [0, 1, 2, 3], [1, 2, 3, 4]]
    assert torsion_indices(mol)[1] == labels[:3]
    # the same residues in two chains are no neighbours
    assert torsion_indices(dict(mol, chain_index=[0] * 7 + [1] * 6), sidechain=True)[1] == ["CHI1 0 PRO 0", "CHI2 0 PRO 0"]
    # the dipeptide of the other trajectory tests: one of each backbone torsion
    assert torsion_indices(dipeptide(), sidechain=True)[1] == ["PHI 0 GLY 1", "PSI 0 ALA 0", "OMEGA 0 ALA 0"]


def test_torsion_indices_without_names_and_without_torsions():
    from jamun_amd.features import ca_distance_indices, torsion_indices

    mol = ace_ala_nme()
    with pytest.raises(ValueError, match="atom names"):
        torsion_indices({k: v for k, v in mol.items() if k != "atom_names"})
    with pytest.raises(ValueError, match="atom names"):
        ca_distance_indices({k: v for k, v in mol.items() if k != "atom_names"})
    single = _mol(["N", "CA", "CB", "C", "O"], ["ALA"] * 5, [0] * 5)
    index, labels = torsion_indices(single, sidechain=True)
    assert index.shape == (0, 4) and index.dtype == np.int32 and labels == []


def test_ca_distance_indices_pair_count_and_separation():
    from jamun_amd.features import ca_distance_indices

    k = 5
    names, res, seq = [], [], []
    for r in range(k):
        names += ["N", "CA", "C", "O"]
        res += ["GLY"] * 4
        seq += [r] * 4
    mol = _mol(names, res, seq)
    index, labels = ca_distance_indices(mol)
    assert index.shape == (math.comb(k, 2), 4) and index.dtype == np.int32 and len(labels) == len(set(labels)) == math.comb(k, 2)
    assert (index[:, 2:] == -1).all() and all(mol["atom_names"][i] == "CA" for i in index[:, :2].ravel())
    assert labels[0] == "CA-CA GLY 0 GLY 1"
    far, _ = ca_distance_indices(mol, min_separation=3)
    assert far.tolist() == [[1, 13, -1, -1], [1, 17, -1, -1], [5, 17, -1, -1]]
    assert ca_distance_indices(mol, min_separation=k)[0].shape == (0, 4)
    assert ca_distance_indices(ace_ala_nme())[0].shape == (0, 4)  # one CA


# ------------------------------------------------------------------------------------------------ the index table of the native call

def test_native_internal_coords_rejects_bad_tables_before_it_needs_a_gpu():
    from jamun_amd import native

    frames = torch.zeros(5, 10, 3)  # (on the CPU: a good table would fail later, for the device)
    for bad in ([[3, -1, 5, -1]], [[0, 10, -1, -1]], [[0, 1, 2, 10]], [[0, -1, -1, -1]], [[-1, -1, -1, -1]], [[0, 1, -2, -1]]):
        with pytest.raises(ValueError, match="index table"):
            native.internal_coords(frames, np.array(bad, dtype=np.int32))
        with pytest.raises(ValueError, match="index table"):
            native.internal_coords(frames, torch.tensor(bad))
    with pytest.raises(ValueError, match="integers"):
        native.internal_coords(frames, np.array([[0.0, 1.0, -1.0, -1.0]]))
    with pytest.raises(ValueError, match="integers"):
        native.internal_coords(frames, torch.tensor([[0.0, 1.0, -1.0, -1.0]]))
    for shape in ((2, 3), (4,), (1, 2, 4)):
        with pytest.raises(ValueError, match=r"\[F, 4\]"):
            native.internal_coords(frames, np.zeros(shape, dtype=np.int64))
    good = native.check_index_table([[0, 1, -1, -1], [9, 8, 7, -1], [0, 1, 2, 3]], 10)
    assert good.dtype == np.int32 and good.flags.c_contiguous and good.shape == (3, 4)
    assert native.check_index_table(np.zeros((0, 4), dtype=np.int64), 10).shape == (0, 4)


def test_feature_tile_constant_mirrors_the_kernels():
    from jamun_amd import native

    hdr = open(os.path.join(ROOT, "jamun_amd", "csrc", "jamun_internal.h")).read()
    assert int(re.search(r"#define JAMUN_INTCOORD_FTILE (\d+)", hdr).group(1)) == native.INTCOORD_FEATURE_TILE


# ---------------------------------------------------------------------------------------------------- the callback on the host path

def _torsion_files(root, chains):
    d = os.path.join(root, "m", "predicted_samples", "torsions")
    return [np.load(os.path.join(d, f"{i}.npy")) for i in range(chains)], np.load(os.path.join(d, "joined.npy"))


@pytest.mark.parametrize("mode,sidechain", [(True, False), ("backbone", False), ("all", True)])
def test_callback_host_path_writes_the_torsion_files(tmp_path, mode, sidechain):
    from jamun_amd.callbacks import SaveTrajectoryCallback
    from jamun_amd.features import internal_coords_host, torsion_indices

    mol = pro_ala()
    n, T, chains = 13, 9, 2
    cpu = torch.device("cpu")
    batches = ic.tumbling_batches(mol, cpu, chains, T, 2, seed=3)
    ds = CaseDataset(mol, "m")
    runs = {}
    for name, kw in (("plain", dict(torsions=mode)), ("superposed", dict(torsions=mode, superpose=True)), ("off", dict())):
        runs[name] = ic.run_callback(SaveTrajectoryCallback([ds], output_dir=str(tmp_path / name), encode="host", async_write=False, **kw), batches, cpu)
    trees = {k: tree(str(tmp_path / k)) for k in runs}
    index, labels = torsion_indices(mol, sidechain=sidechain)
    F = len(labels)
    assert F == (5 if sidechain else 3)
    meta = json.loads(trees["plain"][os.path.join("m", "torsion_labels.json")])
    assert meta["labels"] == labels and meta["atom_indices"] == index.tolist()
    per_chain, joined = _torsion_files(str(tmp_path / "plain"), 2 * chains)
    for c, got in enumerate(per_chain):
        assert got.dtype == np.float32 and got.shape == (T, F)
        frames = batches[c // chains][c % chains]["xhat_traj"].permute(1, 0, 2).numpy()
        assert np.array_equal(got, internal_coords_host(frames, index).astype(np.float32))
    assert joined.dtype == np.float32 and np.array_equal(joined, np.concatenate(per_chain, axis=0)) and joined.shape == (2 * chains * T, F)
    # the same torsion files with superpose on and off; every other file of the plain run is the file of the run without the option
    tors = sorted(f for f in trees["plain"] if "torsion" in f)
    assert len(tors) == 2 * chains + 2 and tors == sorted(f for f in trees["superposed"] if "torsion" in f)
    for f in tors:
        assert trees["plain"][f] == trees["superposed"][f], f
    assert not [f for f in trees["off"] if "torsion" in f]
    assert {f: d for f, d in trees["plain"].items() if "torsion" not in f} == trees["off"]


def test_callback_rejects_unknown_modes_and_molecules_without_names(tmp_path):
    from jamun_amd.callbacks import SaveTrajectoryCallback

    mol = pro_ala()
    with pytest.raises(ValueError, match="torsions must be"):
        SaveTrajectoryCallback([CaseDataset(mol, "m")], output_dir=str(tmp_path), torsions="sidechain")
    with pytest.raises(ValueError, match="atom names"):
        SaveTrajectoryCallback([CaseDataset({k: v for k, v in mol.items() if k != "atom_names"}, "m")], output_dir=str(tmp_path), torsions=True)
    assert SaveTrajectoryCallback([CaseDataset(mol, "m")], output_dir=str(tmp_path), torsions=False).torsions is None


def test_callback_writes_empty_torsion_files_for_a_molecule_without_torsions(tmp_path):
    from jamun_amd.callbacks import SaveTrajectoryCallback

    mol = _mol(["N", "CA", "CB", "C", "O"], ["ALA"] * 5, [0] * 5)
    cpu = torch.device("cpu")
    ic.run_callback(SaveTrajectoryCallback([CaseDataset(mol, "m")], output_dir=str(tmp_path), encode="host", async_write=False, torsions="all"),
                    ic.tumbling_batches(mol, cpu, 2, 4, 1, seed=1), cpu)
    per_chain, joined = _torsion_files(str(tmp_path), 2)
    assert [a.shape for a in per_chain] == [(4, 0)] * 2 and joined.shape == (8, 0) and joined.dtype == np.float32


def test_phi_psi_agree_with_mdtraj(tmp_path):
    """A cross-check only (the analytic cases are the oracle), and only where mdtraj is installed."""
    md = pytest.importorskip("mdtraj")
    from jamun_amd.features import internal_coords_host, torsion_indices
    from jamun_amd.pdb import save_pdb

    mol = dipeptide()
    frames, _, _ = ic.molecule_case("dipeptide")
    path = str(tmp_path / "top.pdb")
    save_pdb(path, mol, mol["pos"][None])
    traj = md.Trajectory(np.array(frames), md.load(path).topology)
    index, labels = torsion_indices(mol)
    (phi_i, phi), (psi_i, psi) = md.compute_phi(traj), md.compute_psi(traj)
    assert index[[l.startswith("PHI") for l in labels]].tolist() == phi_i.tolist() and index[[l.startswith("PSI") for l in labels]].tolist() == psi_i.tolist()
    got = internal_coords_host(frames, index)
    assert np.abs(ic.wrapped(got[:, 0], phi[:, 0])).max() <= 1e-4 and np.abs(ic.wrapped(got[:, 1], psi[:, 0])).max() <= 1e-4
