"""The run of ``SaveTrajectoryCallback(encode="device", superpose=True, torsions="all")`` whose files tests/golden/trajectory_device_trees.json
pins by digest (recorded by tests/golden/make_trajectory_device_trees.py, checked by test_gpu_traj_encode.py): two labels, the 10-atom
dipeptide and a 166-atom chain, 40 frames, three batches of 2 + 1 chains, every value finite and inside the PDB field, so that every
``.pdb``, ``.dcd``, ``rmsd`` and ``torsions`` byte comes from a kernel."""
import hashlib

import torch

from _frames_common import CaseDataset, StubSampler, run, tree
from _traj_molecules import dipeptide, named_chain

T = 40
STAGING_64K = 1 << 16  # at 166 atoms: 32 frames per aligned span and per DCD chunk, a few PDB models per chunk


def molecules() -> dict:
    return {"m": dipeptide(), "c": named_chain(166)}


def batches(dev, mols: dict, n_batches: int = 3):
    """Samples as `unbatch_samples` hands them out: [n, T, 3] views of one [T, sum N, 3] device tensor; the walkers jitter (0.05 nm) around
    their molecule's structure."""
    out = []
    for seed in range(n_batches):
        walkers = ["m", "c", "m"]
        pos = torch.cat([mols[l]["pos"] for l in walkers])
        traj = (pos[None] + 0.05 * torch.randn(T, pos.shape[0], 3, generator=torch.Generator().manual_seed(seed))).to(dev)
        batch, at = [], 0
        for l in walkers:
            n = mols[l]["pos"].shape[0]
            batch.append({"dataset_label": l, "atom_type_index": mols[l]["atom_type_index"], "xhat_traj": traj[:, at : at + n].permute(1, 0, 2)})
            at += n
        out.append(batch)
    return out


def digests(root: str, dev) -> dict:
    """Runs the case into ``root`` -> {relative path: sha256 of the file} after the last batch."""
    from jamun_amd.callbacks import SaveTrajectoryCallback

    mols = molecules()
    cb = SaveTrajectoryCallback([CaseDataset(mols[l], l) for l in mols], output_dir=root, encode="device", superpose=True, torsions="all")
    run(cb, batches(dev, mols), StubSampler(dev))
    assert cb._encoder is not None and not cb._dev_blocks
    return {name: hashlib.sha256(data).hexdigest() for name, data in sorted(tree(root).items())}
