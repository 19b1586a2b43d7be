"""CPU test of ``SaveTrajectoryCallback``'s whole output tree, names and bytes, against the specification of _trajectory_tree.py, after
every batch and for every option that names a file."""
import pytest
import torch

from _frames_common import tree
from _traj_molecules import dipeptide
from _trajectory_tree import expected_tree

T = 4


class _DS:
    def __init__(self, mol, label, xyz=None):
        self.molecule, self._label = mol, label
        if xyz is not None:
            self.xyz = xyz

    def label(self):
        return self._label


class _CpuSampler:
    device = torch.device("cpu"); is_global_zero = True; world_size = 1; global_step = 0


def _datasets(with_xyz: bool = False, only_m: bool = False):
    from jamun_amd import synth

    g = torch.Generator().manual_seed(11)
    m, x = dipeptide(), synth.random_chain(6, seed=4)  # x: a molecule without atom names
    assert "atom_names" in m and "atom_names" not in x
    xyz = {l: (mol["pos"][None] + 0.01 * torch.randn(3, mol["pos"].shape[0], 3, generator=g)) if with_xyz else None for l, mol in (("m", m), ("x", x))}
    return [_DS(m, "m", xyz["m"])] + ([] if only_m else [_DS(x, "x", xyz["x"])])


def _batches(datasets):
    """Two batches of 2 + 1 chains, the labels interleaved (m, x, m); with ``m`` alone its two chains."""
    g = torch.Generator().manual_seed(5)
    by_label = {d.label(): d.molecule for d in datasets}
    out = []
    for _ in range(2):
        batch = []
        for label in ("m", "x", "m"):
            if label in by_label:
                mol = by_label[label]
                pos = mol["pos"][:, None, :] + 0.02 * torch.randn(mol["pos"].shape[0], T, 3, generator=g)
                batch.append({"dataset_label": label, "atom_type_index": mol["atom_type_index"], "xhat_traj": pos})
        out.append(batch)
    return out


CASES = {
    "defaults": ({}, False, False),
    "no_pdb": (dict(write_pdb=False), False, False),
    "no_dcd": (dict(write_dcd=False), False, False),
    "npy_index_restarts": (dict(npy_index_restarts_per_batch=True), False, False),
    "superpose": (dict(superpose=True), True, False),
    "torsions_backbone": (dict(torsions="backbone"), True, False),
    "torsions_all": (dict(torsions="all"), True, False),
    "superpose_torsions_all": (dict(superpose=True, torsions="all"), True, False),
    "true_trajectory": (dict(save_true_trajectory=True), False, False),
    "true_trajectory_xyz": (dict(save_true_trajectory=True), False, True),
    "sync_write": (dict(async_write=False), False, False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_tree_is_the_specified_one_after_every_batch(tmp_path, case):
    from jamun_amd.callbacks import SaveTrajectoryCallback

    options, only_m, with_xyz = CASES[case]
    datasets = _datasets(with_xyz=with_xyz, only_m=only_m)
    batches = _batches(datasets)
    cb = SaveTrajectoryCallback(datasets, output_dir=str(tmp_path / "out"), **options)
    cb.on_sample_start(_CpuSampler())
    assert tree(str(tmp_path / "out")) == expected_tree(datasets, [], options)
    for k in range(len(batches)):
        cb.on_after_sample_batch(batches[k], _CpuSampler())
        cb.flush()
        got, want = tree(str(tmp_path / "out")), expected_tree(datasets, batches[: k + 1], options)
        assert sorted(got) == sorted(want)
        assert [f for f in want if got[f] != want[f]] == []
    cb.on_sample_end(_CpuSampler())
    assert tree(str(tmp_path / "out")) == expected_tree(datasets, batches, options)
    n_m = 4
    assert len(cb.chains["m"]) == cb.num_chains_seen["m"] == n_m
    if case == "true_trajectory":  # no xyz: the named molecule's own structure, nothing for the molecule without names
        assert {f for f in want if "true_samples" in f} == {"m/true_samples/pdb/0.pdb", "m/true_samples/dcd/0.dcd"}
    if case == "true_trajectory_xyz":  # without names there is no .pdb text
        assert {f for f in want if "true_samples" in f} == {"m/true_samples/pdb/0.pdb", "m/true_samples/dcd/0.dcd", "x/true_samples/dcd/0.dcd"}


def test_torsions_refuse_a_molecule_without_atom_names(tmp_path):
    from jamun_amd.callbacks import SaveTrajectoryCallback

    with pytest.raises(ValueError, match="no atom names"):
        SaveTrajectoryCallback(_datasets(), output_dir=str(tmp_path / "out"), superpose=True, torsions="all")
