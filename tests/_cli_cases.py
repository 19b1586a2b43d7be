"""The end-to-end pins of ``jamun_sample`` shared by ``test_cli_cases_host.py`` (CPU) and ``test_gpu_cli.py`` (GPU): the inputs of the three
command-line runs, and `check_run`, which holds every file of a run directory to an oracle fixture of
``tests/golden/make_oracle_fixtures.py`` (``oracle_cli_cfg1``, ``oracle_cli_cfg1_params``, ``oracle_cli_2aa``).

The fixtures were computed from ``jamun_amd.synth`` topologies and the coordinates of the input files read by the generator's own lines,
never through the product's readers, so a reader, collation, config or writer fault shows as a disagreement and cannot cancel out."""
import os
import struct

import numpy as np
import torch

from jamun_amd import synth

from _switch_cases import RMSD_TOL_NM, SIGMA  # noqa: F401  (1e-5 nm, the project's x-hat bound; 0.04 nm, the noise level of both experiments)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INDEX_KEYS = ("atom_type_index", "atom_code_index", "residue_code_index", "residue_sequence_index")

# the dipeptides of test_jamun_sample_uncapped_2aa_directory_end_to_end, in the order the tree is written (a code's seed is its place)
CODES_2AA = ["AG", "GG", "WW", "FY", "KR", "PH", "CM", "DE", "NQ", "ST", "IL", "VA", "RK", "HP", "MC", "ED", "QN", "TS", "LI", "YF",
             "GW", "WA", "AV", "SG", "PP", "KE", "DR", "HH"]
# the command-line overrides of oracle_cli_cfg1_params (make_oracle_fixtures.CLI_PARAMS / CLI_PARAMS_SEED): every parameter its own value
PARAM_OVERRIDES = ["delta=0.05", "friction=0.7", "M=1.3", "inverse_temperature=0.9", "score_fn_clip=40.0", "sigma=0.04", "seed=7"]
PARAM_VALUES = dict(delta=0.05, friction=0.7, M=1.3, inverse_temperature=0.9, score_fn_clip=40.0)


def ag_molecule() -> dict:
    """The AG dipeptide as test_jamun_sample_cfg1_end_to_end writes it to ``uncapped_AG.pdb``."""
    return dict(synth.ag_dipeptide(), elements=["N", "C", "C", "C", "O", "N", "C", "C", "O", "O"], residue_ids=[1] * 5 + [2] * 5)


def molecules_2aa() -> dict:
    """{code: heavy-atom molecule} of the 28-code tree, as ``synth.write_timewarp_tree(root, CODES_2AA)`` builds them."""
    return {code: synth.peptide(code, seed=ci) for ci, code in enumerate(CODES_2AA)}


def load_fixture(name: str) -> dict:
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def fixture_codes(fx: dict) -> list:
    return ["".join(chr(c) for c in row) for row in fx["codes"]]


def labels_2aa(fx: dict) -> dict:
    """label -> (first walker, end walker) of the 2AA batch: one walker per code, in the fixture's (sorted) order."""
    return {code: (w, w + 1) for w, code in enumerate(fixture_codes(fx))}


def walker_inputs(fx: dict, w: int) -> dict:
    """What the oracle consumed for walker ``w``: pos, the four index tensors and its bonds as a set of directed (lower, upper) pairs."""
    a, b = int(fx["ptr"][w]), int(fx["ptr"][w + 1])
    out = {k: fx[k][a:b] for k in ("pos",) + INDEX_KEYS}
    mine = (fx["bonds"][0] >= a) & (fx["bonds"][0] < b)
    out["bonds"] = sorted(map(tuple, (fx["bonds"][:, mine] - a).T.tolist()))
    return out


def n_batches(fx: dict) -> int:
    return sum(1 for k in fx if k.startswith("xhat_traj_"))


def read_dcd(path: str):
    """Minimal CHARMM DCD record parser (little-endian Fortran records; the repository ships a writer only): the header's frame count,
    the atom count record and per frame the X, Y, Z float32 records -> float32 [frames, atoms, 3] in the file's unit (Angstrom)."""
    b = open(path, "rb").read()
    o = 0

    def rec():
        nonlocal o
        n = struct.unpack_from("<i", b, o)[0]
        body = b[o + 4 : o + 4 + n]
        assert len(body) == n and struct.unpack_from("<i", b, o + 4 + n)[0] == n, f"{path}: record markers disagree at byte {o}"
        o += n + 8
        return body

    head = rec()
    assert len(head) == 84 and head[:4] == b"CORD", path
    nset = struct.unpack_from("<i", head, 4)[0]
    rec()  # titles
    natom = struct.unpack("<i", rec())[0]
    frames = np.empty((nset, natom, 3), dtype=np.float32)
    for t in range(nset):
        for c in range(3):
            frames[t, :, c] = np.frombuffer(rec(), dtype="<f4")
    assert o == len(b), f"{path}: {len(b) - o} bytes behind the last of {nset} frames"
    return frames


def read_pdb_models(path: str):
    """[(names, residue names, residue ids, float64 [n, 3] Angstrom as printed)] per MODEL of a multi-model PDB file."""
    models, cur = [], None
    for line in open(path):
        if line.startswith("MODEL"):
            cur = ([], [], [], [])
            models.append(cur)
        elif line.startswith("ATOM  "):
            if cur is None:  # (a single structure without MODEL records)
                cur = ([], [], [], [])
                models.append(cur)
            cur[0].append(line[12:16].strip())
            cur[1].append(line[17:20].strip())
            cur[2].append(int(line[22:26]))
            cur[3].append([float(line[30:38]), float(line[38:46]), float(line[46:54])])
    return [(m[0], m[1], m[2], np.asarray(m[3], dtype=np.float64).reshape(-1, 3)) for m in models]


def _angstrom(frames_nm: np.ndarray) -> np.ndarray:
    """float32 nm -> float32 Angstrom by ONE float32 multiply: the encoders' documented arithmetic (``coord * 10.0f`` in
    jamun_traj.hip's k_encode_dcd / k_encode_pdb, ``xyz * np.float32(10.0)`` in pdb.save_dcd, ``frames[t] * 10`` on a float32 tensor in
    pdb.save_pdb), so the DCD comparison below is bit equality and not a 1 ulp band."""
    assert frames_nm.dtype == np.float32
    return frames_nm * np.float32(10.0)


def _check_pdb(path: str, mol: dict, frames_nm: np.ndarray, what: str) -> None:
    """frames_nm [T, n, 3]: MODEL count, per model the molecule's atom names / residue names / residue ids, coordinates to the format's
    0.001 Angstrom: half a unit of the last printed digit plus one float32 ulp of the value."""
    models = read_pdb_models(path)
    assert len(models) == frames_nm.shape[0], (what, "models", len(models), frames_nm.shape[0])
    want = _angstrom(frames_nm)
    for t, (names, resn, resid, xyz) in enumerate(models):
        assert names == list(mol["atom_names"]), (what, t, "atom names")
        assert resn == list(mol["residues"]), (what, t, "residue names")
        assert resid == [int(i) for i in mol["residue_ids"]], (what, t, "residue ids")
        assert xyz.shape == want[t].shape, (what, t, xyz.shape)
        excess = np.abs(xyz - want[t].astype(np.float64)) - (0.0005 + np.spacing(np.abs(want[t])).astype(np.float64))
        assert excess.max() <= 0.0, (what, t, "coordinates", float(excess.max()))


def check_topology(run_dir: str, label: str, mol: dict, pos_nm: np.ndarray) -> None:
    """``sampler/<label>/topology.pdb`` holds the input structure: the molecule's atoms in order at the positions the oracle started from."""
    _check_pdb(os.path.join(run_dir, "sampler", label, "topology.pdb"), mol, np.asarray(pos_nm, dtype=np.float32)[None], f"{label}/topology.pdb")


def frame_rmsd(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """[n, T, 3] x 2 -> per-frame RMSD [T] (float64)."""
    return np.sqrt(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum(-1).mean(0))


def check_run(run_dir: str, fx: dict, labels: dict, molecules: dict, report: dict = None) -> float:
    """Hold every file under ``<run_dir>/sampler/<label>/`` to the fixture ``fx``.  ``labels``: label -> (first walker, end walker) of the
    fixture's batch (``ptr``); ``molecules``: label -> the input molecule (atom names, residue names, residue ids).  Returns the worst
    per-frame RMSD in nm (also ``report[label]`` when given); raises AssertionError at the first file that disagrees.

    Numbers: chain ``i = walkers_of_label * b + w`` is walker ``w`` of batch ``b``.  Its ``.npy`` is the oracle's ``xhat_traj_b`` slice as
    ``[n, T, 3]`` to RMSD_TOL_NM per frame, the project's bar (BASELINE.json), and — so that one misplaced atom of a frame cannot hide in
    the mean over the others — with no atom further than RMSD_TOL_NM from the oracle's: the same number in the stricter norm.  Everything
    else is exact: ``joined.npy`` is the chain files concatenated, the DCD files are the ``.npy`` x 10 bit for bit (`_angstrom`), the PDB
    files are the ``.npy`` x 10 to the printed digit."""
    worst = 0.0
    nb = n_batches(fx)
    for label, (lo, hi) in labels.items():
        nw = hi - lo
        mol = molecules[label]
        base = os.path.join(run_dir, "sampler", label, "predicted_samples")
        check_topology(run_dir, label, mol, walker_inputs(fx, lo)["pos"])
        chains = []
        worst_label = 0.0
        for b in range(nb):
            ref_batch = fx[f"xhat_traj_{b}"]  # [T, N, 3]
            for w in range(nw):
                i = nw * b + w
                a0, a1 = int(fx["ptr"][lo + w]), int(fx["ptr"][lo + w + 1])
                ref = np.transpose(ref_batch[:, a0:a1], (1, 0, 2))  # "frames atoms coords -> atoms frames coords"
                got = np.load(os.path.join(base, "npy", f"{i}.npy"))
                assert got.dtype == np.float32 and got.shape == ref.shape, (label, i, got.dtype, got.shape, ref.shape)
                assert np.isfinite(got).all(), (label, i)
                r = frame_rmsd(got, ref)
                far = np.sqrt(((got.astype(np.float64) - ref.astype(np.float64)) ** 2).sum(-1)).max()
                worst_label = max(worst_label, float(r.max()))
                assert r.max() <= RMSD_TOL_NM, (label, "chain", i, "frame", int(r.argmax()), "rmsd", float(r.max()))
                assert far <= RMSD_TOL_NM, (label, "chain", i, "one atom", float(far))
                frames = np.ascontiguousarray(np.transpose(got, (1, 0, 2)))  # [T, n, 3]
                d = read_dcd(os.path.join(base, "dcd", f"{i}.dcd"))
                assert d.shape == frames.shape, (label, i, "dcd", d.shape, frames.shape)
                assert np.array_equal(d, _angstrom(frames)), (label, i, "dcd is not the .npy x 10", float(np.abs(d - _angstrom(frames)).max()))
                _check_pdb(os.path.join(base, "pdb", f"{i}.pdb"), mol, frames, f"{label}/pdb/{i}.pdb")
                chains.append(got)
        assert not os.path.exists(os.path.join(base, "npy", f"{nw * nb}.npy")), (label, "more chains than walkers x batches")
        joined = np.load(os.path.join(base, "npy", "joined.npy"))
        want = np.concatenate(chains, axis=1)  # "b n t c -> n (b t) c" in chain order
        assert joined.dtype == np.float32 and joined.shape == want.shape, (label, "joined.npy", joined.shape, want.shape)
        assert np.array_equal(joined, want), (label, "joined.npy is not the chain files in chain order")
        jf = np.ascontiguousarray(np.transpose(joined, (1, 0, 2)))
        d = read_dcd(os.path.join(base, "dcd", "joined.dcd"))
        assert d.shape == jf.shape, (label, "joined.dcd", d.shape, jf.shape)
        assert np.array_equal(d, _angstrom(jf)), (label, "joined.dcd is not joined.npy x 10")
        _check_pdb(os.path.join(base, "pdb", "joined.pdb"), mol, jf, f"{label}/pdb/joined.pdb")
        if report is not None:
            report[label] = worst_label
        worst = max(worst, worst_label)
    return worst


def write_run_from_fixture(run_dir: str, fx: dict, labels: dict, molecules: dict, chains_of=None, joined_of=None, frames_for_dcd=None) -> None:
    """A correct run directory made from the fixture itself with the product's host writers (np.save, pdb.save_pdb, pdb.save_dcd) — the
    starting point of the checker's must-fail mutations.  The hooks replace one stage: ``chains_of(label, chains)`` the list of chain
    arrays [n, T, 3] in file order, ``joined_of(label, chains)`` the joined array, ``frames_for_dcd(frames)`` what the DCD writer gets."""
    from jamun_amd import pdb

    nb = n_batches(fx)
    for label, (lo, hi) in labels.items():
        mol = dict(molecules[label])
        mol.setdefault("elements", [n[0] for n in mol["atom_names"]])
        base = os.path.join(run_dir, "sampler", label, "predicted_samples")
        for ext in ("npy", "pdb", "dcd"):
            os.makedirs(os.path.join(base, ext), exist_ok=True)
        pdb.save_pdb(os.path.join(run_dir, "sampler", label, "topology.pdb"), mol, torch.from_numpy(walker_inputs(fx, lo)["pos"])[None])
        chains = []
        for b in range(nb):
            for w in range(lo, hi):
                a0, a1 = int(fx["ptr"][w]), int(fx["ptr"][w + 1])
                chains.append(np.ascontiguousarray(np.transpose(fx[f"xhat_traj_{b}"][:, a0:a1], (1, 0, 2))))
        if chains_of is not None:
            chains = chains_of(label, chains)
        joined = np.concatenate(chains, axis=1) if joined_of is None else joined_of(label, chains)
        for name, arr in [(str(i), c) for i, c in enumerate(chains)] + [("joined", joined)]:
            np.save(os.path.join(base, "npy", name + ".npy"), arr)
            if arr.ndim != 3 or arr.shape[0] != len(mol["atom_names"]):
                continue  # (a mutation that no molecule file can hold: the .npy alone must be refused)
            frames = np.ascontiguousarray(np.transpose(arr, (1, 0, 2)))
            pdb.save_pdb(os.path.join(base, "pdb", name + ".pdb"), mol, frames)
            pdb.save_dcd(os.path.join(base, "dcd", name + ".dcd"), frames if frames_for_dcd is None else frames_for_dcd(frames))
