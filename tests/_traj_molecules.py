"""Molecules with atom names for the trajectory-encoder tests (test_traj_encode_host.py, test_gpu_traj_encode.py)."""
import torch

from jamun_amd import synth


def dipeptide() -> dict:
    """The hand-built Ala-Gly dipeptide: two residues, nine bonds (a CONECT block with one to three partners per atom)."""
    return dict(synth.ag_dipeptide(), elements=["N", "C", "C", "C", "O", "N", "C", "C", "O", "O"], residue_ids=[1] * 5 + [2] * 5)


def named_chain(n_atoms: int, seed: int = 0) -> dict:
    """`synth.random_chain` with names attached: atom names of one to four characters, residues of five atoms, two chains."""
    mol = synth.random_chain(n_atoms, seed=seed)
    els = [["C", "O", "N"][int(t)] for t in mol["atom_type_index"]]
    res_names = ["ALA", "GLY", "SER", "TRP", "LYS"]
    return dict(mol, atom_names=[(els[i] + ["", "A", "G1", "XT2"][i % 4])[:4] for i in range(n_atoms)], elements=els,
                residues=[res_names[(i // 5) % 5] for i in range(n_atoms)], residue_ids=[i // 5 + 1 for i in range(n_atoms)],
                chain_index=[0 if i < (n_atoms + 1) // 2 else 1 for i in range(n_atoms)])


def one_atom() -> dict:
    return dict(pos=torch.zeros(1, 3), atom_type_index=torch.zeros(1, dtype=torch.int32), atom_code_index=torch.zeros(1, dtype=torch.int32),
                residue_code_index=torch.zeros(1, dtype=torch.int32), residue_sequence_index=torch.zeros(1, dtype=torch.int32),
                bonds=torch.zeros((2, 0), dtype=torch.long), atom_names=["CA"], residues=["GLY"], elements=["C"], residue_ids=[1])


def molecule(n_atoms: int) -> dict:
    return one_atom() if n_atoms == 1 else dipeptide() if n_atoms == 10 else named_chain(n_atoms)


def fill_template(body: bytes, offsets, frames: torch.Tensor, first_model: int = 0) -> bytes:
    """Model text from a `pdb.pdb_model_template`: the MODEL line, then the body with f"{v:8.3f}" of v = fp32(x * 10) in each field."""
    out = []
    for t in range(frames.shape[0]):
        b = bytearray(body)
        xyz = (frames[t].float() * 10).tolist()
        for i, off in enumerate(offsets.tolist()):
            b[off : off + 24] = "".join(f"{v:8.3f}" for v in xyz[i]).encode()
        out.append(f"MODEL        {first_model + t}\n".encode() + bytes(b))
    return b"".join(out)
