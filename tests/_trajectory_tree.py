"""The files ``SaveTrajectoryCallback`` leaves behind, written out from its class docstring with the primitives alone (`np.save`,
`pdb.save_pdb`, `pdb.save_dcd`, `superpose.superpose_host`, `features.torsion_indices`, `features.internal_coords_host`, `json`): the
specification test_trajectory_tree_host.py holds the callback to.  Nothing here uses the callback."""
import json
import os
import tempfile

import numpy as np

from _frames_common import tree

OPTIONS = dict(sample_key="xhat_traj", write_pdb=True, write_dcd=True, save_true_trajectory=False, npy_index_restarts_per_batch=False,
               superpose=False, torsions=False)


def _named(ds):
    mol = getattr(ds, "molecule", None)
    return mol if mol is not None and "atom_names" in mol else None


def _write_start(root: str, ds, opt: dict) -> None:
    """What exists before the first batch: ``topology.pdb``, ``torsion_labels.json``, ``true_samples/{pdb,dcd}/0.*``."""
    from jamun_amd.features import torsion_indices
    from jamun_amd.pdb import save_dcd, save_pdb

    mol = _named(ds)
    if opt["torsions"]:
        index, labels = torsion_indices(ds.molecule, backbone=True, sidechain=opt["torsions"] == "all")
        with open(os.path.join(root, "torsion_labels.json"), "w") as f:
            json.dump({"labels": labels, "atom_indices": index.tolist(), "unit": "rad"}, f, indent=1)
    if mol is not None and opt["write_pdb"]:
        save_pdb(os.path.join(root, "topology.pdb"), mol, mol["pos"][None])
    if not opt["save_true_trajectory"]:
        return
    xyz = getattr(ds, "xyz", None)
    if xyz is None and mol is None:
        return  # (neither frames nor names: no true samples)
    frames = (xyz if xyz is not None else mol["pos"][None]).detach().cpu().numpy()
    for ext in ("pdb", "dcd"):
        os.makedirs(os.path.join(root, "true_samples", ext), exist_ok=True)
    if mol is not None:
        save_pdb(os.path.join(root, "true_samples", "pdb", "0.pdb"), mol, frames)
    save_dcd(os.path.join(root, "true_samples", "dcd", "0.dcd"), frames)


def _write_trajectory(pred: str, name, npy_name, arr: np.ndarray, ds, opt: dict) -> None:
    """``arr`` [n, T', 3] nm as ``<name>.*``: the raw ``.npy``, the torsions of the raw frames, and the frames (superposed on the dataset
    molecule's ``pos`` with ``superpose``, whose RMSD is a file too) as ``.pdb`` models and ``.dcd`` records."""
    from jamun_amd.features import internal_coords_host, torsion_indices
    from jamun_amd.pdb import save_dcd, save_pdb
    from jamun_amd.superpose import superpose_host

    def path(kind, stem, ext):
        os.makedirs(os.path.join(pred, kind), exist_ok=True)
        return os.path.join(pred, kind, f"{stem}.{ext}")

    np.save(path("npy", npy_name, "npy"), arr)
    frames = np.transpose(arr, (1, 0, 2))
    if opt["torsions"]:
        index, _ = torsion_indices(ds.molecule, backbone=True, sidechain=opt["torsions"] == "all")
        np.save(path("torsions", name, "npy"), internal_coords_host(frames, index).astype(np.float32))
    if opt["superpose"]:
        ref = np.ascontiguousarray(ds.molecule["pos"].detach().cpu().numpy(), dtype=np.float32)
        frames, rmsd = superpose_host(frames, ref)
        np.save(path("rmsd", name, "npy"), rmsd)
    mol = _named(ds)
    if opt["write_pdb"] and mol is not None:
        save_pdb(path("pdb", name, "pdb"), mol, frames)
    if opt["write_dcd"]:
        save_dcd(path("dcd", name, "dcd"), frames)


def expected_tree(datasets, batches_so_far, options) -> dict:
    """{relative path: bytes} under the callback's ``output_dir`` after ``on_sample_start`` and the batches of ``batches_so_far`` (each a
    list of samples ``{"dataset_label", <sample_key>: [n, T, 3]}``), for the constructor ``options`` that name files."""
    opt = dict(OPTIONS, **{k: v for k, v in options.items() if k in OPTIONS})
    opt["torsions"] = {None: False, False: False, True: "backbone", "backbone": "backbone", "all": "all"}[opt["torsions"]]
    by_label = {}
    for ds in datasets:
        by_label.setdefault(ds.label(), ds)
    with tempfile.TemporaryDirectory() as root:
        for label in sorted(by_label):
            ds = by_label[label]
            pred = os.path.join(root, label, "predicted_samples")
            for ext in ("npy", "pdb", "dcd"):
                os.makedirs(os.path.join(pred, ext), exist_ok=True)
            _write_start(os.path.join(root, label), ds, opt)
            chains = []
            for batch in batches_so_far:
                new = [np.ascontiguousarray(s[opt["sample_key"]].detach().cpu().numpy()) for s in batch if s["dataset_label"] == label]
                if not new:
                    continue
                for k, arr in enumerate(new):  # (.npy: the running index too, unless the reference's numbering is asked for)
                    i = len(chains) + k
                    _write_trajectory(pred, i, k if opt["npy_index_restarts_per_batch"] else i, arr, ds, opt)
                chains.extend(new)
                _write_trajectory(pred, "joined", "joined", np.concatenate(chains, axis=1), ds, opt)  # "b n t c -> n (b t) c"
        return tree(root)
