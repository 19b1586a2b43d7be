"""CPU tests of the trajectory encoder's host side: the per-molecule PDB template, the size function of the C ABI, the append helpers
and the callback's ``encode`` switch.  `pdb.save_pdb` / `pdb.save_dcd` are the specification throughout."""
import ctypes as C
import filecmp
import os
import re

import numpy as np
import pytest
import torch

from _traj_molecules import dipeptide, fill_template, named_chain, one_atom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["jamun_pdb_models_nbytes", "jamun_encode_pdb_models", "jamun_encode_dcd_frames"]


def _saved(tmp_path, mol, frames, name="ref.pdb") -> bytes:
    from jamun_amd import pdb

    path = str(tmp_path / name)
    pdb.save_pdb(path, mol, frames)
    return open(path, "rb").read()


@pytest.mark.parametrize("make", [dipeptide, one_atom, lambda: named_chain(166)], ids=["dipeptide", "one_atom", "chain166"])
def test_template_filled_in_python_reproduces_save_pdb(tmp_path, make):
    from jamun_amd import pdb

    mol = make()
    n = len(mol["atom_names"])
    body, off = pdb.pdb_model_template(mol)
    assert off.dtype == np.int32 and off.shape == (n,) and np.all(np.diff(off) > 0)
    assert body.endswith(b"ENDMDL\n") and body.count(b"CONECT") == n
    g = torch.Generator().manual_seed(n)
    frames = torch.randn(12, n, 3, generator=g) * torch.tensor([0.01, 1.0, 30.0])  # one to three digits in front of the point, both signs
    assert fill_template(body, off, frames) + b"END\n" == _saved(tmp_path, mol, frames)


def test_pdb_models_nbytes_is_the_length_of_the_real_text():
    from jamun_amd import native, pdb

    body, _ = pdb.pdb_model_template(dipeptide())
    for first in (0, 9, 10, 99, 99_999):
        for n_frames in (1, 2, 11, 1000):
            text = b"".join(f"MODEL        {t}\n".encode() + body for t in range(first, first + n_frames))
            assert native.pdb_models_nbytes(len(body), first, n_frames) == len(text), (first, n_frames)
    assert native.pdb_models_nbytes(len(body), 5, 0) == 0


def test_appends_equal_one_save_of_all_frames(tmp_path):
    """Three appends of host-formatted models / records = one save_pdb / save_dcd of the concatenation; the middle append crosses the
    model numbers 9 -> 10 (the MODEL line grows by one character)."""
    from jamun_amd import pdb

    mol = dipeptide()
    n = 10
    body, off = pdb.pdb_model_template(mol)
    frames = torch.randn(25, n, 3, generator=torch.Generator().manual_seed(3))
    cuts = [0, 7, 13, 25]
    p, d = str(tmp_path / "a.pdb"), str(tmp_path / "a.dcd")
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        pdb.append_pdb_models(p, fill_template(body, off, frames[lo:hi], first_model=lo))
        ang = np.transpose(frames[lo:hi].numpy() * np.float32(10.0), (0, 2, 1))
        recs = np.empty((hi - lo, 3), dtype=np.dtype([("a", "<i4"), ("v", "<f4", (n,)), ("b", "<i4")]))
        recs["a"] = recs["b"] = 4 * n
        recs["v"] = ang
        pdb.append_dcd_frames(d, n, recs.tobytes(), hi - lo)
        # after every append the files are what the host writers give for the frames so far
        assert open(p, "rb").read() == _saved(tmp_path, mol, frames[:hi])
        pdb.save_dcd(str(tmp_path / "ref.dcd"), frames[:hi])
        assert filecmp.cmp(d, str(tmp_path / "ref.dcd"), shallow=False)
    with pytest.raises(ValueError):
        pdb.append_dcd_frames(d, n, b"\0" * 12, 1)  # not one frame of 10 atoms
    with pytest.raises(ValueError):
        pdb.append_dcd_frames(d, n + 1, b"\0" * (3 * (4 * (n + 1) + 8)), 1)  # another molecule's file
    open(str(tmp_path / "broken.pdb"), "wb").write(b"MODEL        0\n")
    with pytest.raises(ValueError):
        pdb.append_pdb_models(str(tmp_path / "broken.pdb"), b"")


def _trees_equal(a: str, b: str) -> None:
    fa = sorted(os.path.relpath(os.path.join(dp, f), a) for dp, _, fs in os.walk(a) for f in fs)
    fb = sorted(os.path.relpath(os.path.join(dp, f), b) for dp, _, fs in os.walk(b) for f in fs)
    assert fa == fb and fa
    for f in fa:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f


def test_callback_encode_switch_on_cpu_tensors(tmp_path):
    from jamun_amd.callbacks import SaveTrajectoryCallback

    mol = dipeptide()

    class DS:
        molecule = mol

        def label(self):
            return "m"

    class FakeSampler:
        device = torch.device("cpu"); is_global_zero = True; world_size = 1; global_step = 0

    g = torch.Generator().manual_seed(0)
    batches = [[{"dataset_label": "m", "xhat_traj": torch.randn(10, 4, 3, generator=g)} for _ in range(2)] for _ in range(2)]
    with pytest.raises(ValueError, match="encode"):
        SaveTrajectoryCallback([DS()], output_dir=str(tmp_path / "x"), encode="gpu")
    for mode in ("auto", "host"):
        cb = SaveTrajectoryCallback([DS()], output_dir=str(tmp_path / mode), encode=mode)
        cb.on_sample_start(FakeSampler())
        for b in batches:
            cb.on_after_sample_batch(b, FakeSampler())
        cb.on_sample_end(FakeSampler())
        assert len(cb.chains["m"]) == 4
    _trees_equal(str(tmp_path / "auto"), str(tmp_path / "host"))
    assert os.path.exists(str(tmp_path / "auto" / "m" / "predicted_samples" / "pdb" / "joined.pdb"))
    cb = SaveTrajectoryCallback([DS()], output_dir=str(tmp_path / "device"), encode="device")
    with pytest.raises(RuntimeError, match="GPU"):
        cb.on_after_sample_batch(batches[0], FakeSampler())
    cb.close()


def test_new_symbols_are_declared_bound_and_exported():
    from jamun_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jamun_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.jamun_version() == 6  # additive: no struct changed


def test_argument_errors_are_reported_without_a_gpu():
    from jamun_amd import _lib

    lib = _lib.load()
    INVALID = -1
    nb = C.c_int64()
    assert lib.jamun_pdb_models_nbytes(100, 0, 1, None) == INVALID and b"null" in lib.jamun_last_error()
    assert lib.jamun_pdb_models_nbytes(-1, 0, 1, C.byref(nb)) == INVALID and b"negative" in lib.jamun_last_error()
    assert lib.jamun_pdb_models_nbytes(100, -1, 1, C.byref(nb)) == INVALID
    assert lib.jamun_pdb_models_nbytes(100, 0, -1, C.byref(nb)) == INVALID
    p = 4096  # (never dereferenced: every call below fails its argument checks before any device work)
    pdb_ok = dict(xyz=p, fs=30, as_=3, n=10, T=2, first=0, body=p, body_len=100, off=p, out=p, cap=10_000, cnt=p)

    def enc_pdb(**over):
        a = dict(pdb_ok, **over)
        return lib.jamun_encode_pdb_models(a["xyz"], a["fs"], a["as_"], a["n"], a["T"], a["first"], a["body"], a["body_len"], a["off"], a["out"],
                                           a["cap"], a["cnt"], None)

    for null in ("xyz", "body", "off", "out", "cnt"):
        assert enc_pdb(**{null: None}) == INVALID and b"null" in lib.jamun_last_error(), null
    for neg in ("fs", "as_", "n", "T", "first", "body_len", "cap"):
        assert enc_pdb(**{neg: -1}) == INVALID, neg
    assert enc_pdb(cap=2 * (14 + 1 + 100) - 1) == INVALID and b"too small" in lib.jamun_last_error()  # two models of 115 bytes
    assert enc_pdb(n=99_999) == INVALID and b"serial" in lib.jamun_last_error()
    with pytest.raises(RuntimeError, match="jamun_hip error -1"):
        _lib.check(enc_pdb(n=99_999))

    def enc_dcd(xyz=p, fs=30, as_=3, n=10, T=2, out=p, cap=10_000):
        return lib.jamun_encode_dcd_frames(xyz, fs, as_, n, T, out, cap, None)

    assert enc_dcd(xyz=None) == INVALID and enc_dcd(out=None) == INVALID
    for neg in ("fs", "as_", "n", "T", "cap"):
        assert enc_dcd(**{neg: -1}) == INVALID, neg
    assert enc_dcd(cap=2 * 3 * 48 - 1) == INVALID and b"too small" in lib.jamun_last_error()
