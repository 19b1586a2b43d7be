"""GPU tests of the trajectory encoders (jamun_traj.hip) and of ``SaveTrajectoryCallback(encode="device")``.  The expected bytes always
come from `pdb.save_pdb` / `pdb.save_dcd` (MODEL lines renumbered for a late ``first_model``), never from the encoder."""
import filecmp
import json
import os
import re
import time

import numpy as np
import pytest
import torch

import _trajectory_device_case as case
from _frames_common import _dev
from _traj_molecules import molecule, named_chain

pytestmark = pytest.mark.gpu

DCD_PREAMBLE = 276  # bytes of a save_dcd file in front of the coordinate records: header, title block, atom count


def _expected_models(tmp_path, mol, frames: torch.Tensor, first_model: int) -> bytes:
    """Model text of ``frames`` [T, n, 3] numbered from ``first_model``, from save_pdb: for a small ``first_model`` literally the tail of a
    longer file (zero frames in front), else save_pdb's text with the MODEL lines renumbered."""
    from jamun_amd import pdb

    path = str(tmp_path / "expected.pdb")
    if first_model <= 16:
        pad = torch.zeros((first_model,) + tuple(frames.shape[1:]))
        pdb.save_pdb(path, mol, torch.cat([pad, frames.cpu().float()]))
        txt = open(path, "rb").read()
        at = txt.index(f"MODEL        {first_model}\n".encode())
        assert txt.endswith(b"END\n")
        return txt[at:-4]
    pdb.save_pdb(path, mol, frames)
    txt = open(path, "rb").read()[:-4]
    return re.sub(rb"^MODEL        (\d+)\n", lambda m: b"MODEL        %d\n" % (int(m.group(1)) + first_model), txt, flags=re.M)


def _layouts(frames: torch.Tensor, layout: str, dev) -> torch.Tensor:
    """``frames`` [T, n, 3] on the device as a [T, n, 3] VIEW of one of the two trajectory layouts (no copy inside the encoder)."""
    T, n, _ = frames.shape
    if layout == "frame_major":  # a molecule's slice of [T, sum N, 3]
        big = torch.full((T, n + 7, 3), float("nan"), device=dev)
        big[:, 3 : 3 + n] = frames.to(dev)
        view = big[:, 3 : 3 + n]
    else:  # contiguous [n, T, 3]
        view = frames.to(dev).transpose(0, 1).contiguous().transpose(0, 1)
        assert view.stride() == (3, 3 * T, 1) or T == 1 or n == 1
    assert view.shape == (T, n, 3)
    return view


def _encode_pdb(mol, view: torch.Tensor, first_model: int, misalign: int = 0):
    from jamun_amd import native, pdb

    dev = view.device
    body, off = pdb.pdb_model_template(mol)
    body_d = torch.frombuffer(bytearray(body), dtype=torch.uint8).to(dev)
    off_d = torch.from_numpy(off).to(dev)
    need = native.pdb_models_nbytes(len(body), first_model, view.shape[0])
    guard = 64
    buf = torch.full((misalign + need + guard,), 0xAB, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    got = native.encode_pdb_models(view, first_model, body_d, off_d, buf[misalign : misalign + need], cnt)
    torch.cuda.synchronize()
    assert got == need
    host = buf.cpu().numpy()
    assert (host[:misalign] == 0xAB).all() and (host[misalign + need :] == 0xAB).all()  # nothing outside the exact size
    return host[misalign : misalign + need].tobytes(), int(cnt.item())


@pytest.mark.parametrize("layout", ["frame_major", "atom_major"])
@pytest.mark.parametrize("T", [1, 7, 1500])
@pytest.mark.parametrize("n", [1, 10, 29, 166])
def test_pdb_bytes_equal_save_pdb(tmp_path, n, T, layout):
    dev = _dev()
    mol = molecule(n)
    frames = torch.randn(T, n, 3, generator=torch.Generator().manual_seed(1000 * n + T))  # N(0, 1) nm
    got, bad = _encode_pdb(mol, _layouts(frames, layout, dev), 0, misalign=(n + T) % 16)
    assert bad == 0
    assert got == _expected_models(tmp_path, mol, frames, 0)


@pytest.mark.parametrize("first_model,T", [(5, 7), (9, 2), (99_995, 12), (99_999, 1), (100_000, 3)])
@pytest.mark.parametrize("n", [10, 29])
def test_pdb_model_numbers_across_a_new_digit(tmp_path, n, first_model, T):
    dev = _dev()
    mol = molecule(n)
    frames = torch.randn(T, n, 3, generator=torch.Generator().manual_seed(first_model + n))
    got, bad = _encode_pdb(mol, _layouts(frames, "frame_major", dev), first_model, misalign=3)
    assert bad == 0
    want = _expected_models(tmp_path, mol, frames, first_model)
    assert want.startswith(f"MODEL        {first_model}\n".encode()) and f"MODEL        {first_model + T - 1}\n".encode() in want
    assert got == want


def _exact_ties() -> np.ndarray:
    """float32 inputs x (nm) whose Angstrom value v = fp32(x * 10) times 1000 is an exact half (v = j / 16 with j odd: 62.5 j), found by
    brute force over the neighbourhood of j / 160."""
    found = []
    for j in range(1, 1200, 2):
        for sign in (1.0, -1.0):
            x = np.float32(sign * j / 160.0)
            for cand in (np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))):
                v = np.float32(cand) * np.float32(10.0)
                if abs(float(v) * 1000.0) % 1.0 == 0.5:
                    found.append(np.float32(cand))
    return np.unique(np.array(found, dtype=np.float32))


def test_pdb_rounding_ties_signed_zero_and_width_boundary(tmp_path):
    dev = _dev()
    ties = _exact_ties()
    assert len(ties) >= 100 and (ties < 0).sum() >= 40 and (ties > 0).sum() >= 40
    special = np.array([0.0, -0.0, -1e-5, 1e-5, 999.9999, -99.9999, 0.00005, -0.00005, 99.99995, 0.1, -0.1], dtype=np.float32)
    vals = np.concatenate([ties, special])
    n = 10
    T = -(-len(vals) // (3 * n)) + 1
    flat = np.resize(vals, T * n * 3).astype(np.float32)
    frames = torch.from_numpy(flat.reshape(T, n, 3).copy())
    mol = molecule(n)
    for layout in ("frame_major", "atom_major"):
        got, bad = _encode_pdb(mol, _layouts(frames, layout, dev), 0, misalign=5)
        assert bad == 0
        want = _expected_models(tmp_path, mol, frames, 0)
        assert b"  -0.000" in want and b"9999.999" in want and b"-999.999" in want
        assert got == want


def test_unencodable_values_are_counted_exactly():
    dev = _dev()
    n, T = 10, 9
    mol = molecule(n)
    frames = torch.randn(T, n, 3, generator=torch.Generator().manual_seed(7))
    frames[0, 0, 0] = float("nan")
    frames[3, 9, 2] = float("inf")
    frames[3, 2, 1] = float("-inf")
    frames[8, 5, 1] = 1000.0   # 10000.000 Angstrom: nine characters
    frames[8, 5, 2] = -100.0   # -1000.000
    got, bad = _encode_pdb(mol, _layouts(frames, "frame_major", dev), 0)
    assert bad == 5
    # the placeholder keeps the file well formed: every coordinate field still parses
    for line in got.decode().splitlines():
        if line.startswith("ATOM"):
            [float(line[30 + 8 * c : 38 + 8 * c]) for c in range(3)]
    clean = torch.randn(T, n, 3, generator=torch.Generator().manual_seed(8))
    assert _encode_pdb(mol, _layouts(clean, "atom_major", dev), 0)[1] == 0


@pytest.mark.parametrize("layout", ["frame_major", "atom_major"])
@pytest.mark.parametrize("n,T", [(1, 1), (10, 7), (29, 1500), (166, 33)])
def test_dcd_records_equal_save_dcd_payload(tmp_path, n, T, layout):
    from jamun_amd import native, pdb

    dev = _dev()
    frames = torch.randn(T, n, 3, generator=torch.Generator().manual_seed(n * T))
    frames[0, 0, 0] = -0.0
    path = str(tmp_path / "ref.dcd")
    pdb.save_dcd(path, frames)
    want = open(path, "rb").read()[DCD_PREAMBLE:]
    need = T * 3 * (4 * n + 8)
    assert len(want) == need
    for misalign in (0, 4):
        buf = torch.full((misalign + need + 64,), 0xAB, dtype=torch.uint8, device=dev)
        assert native.encode_dcd_frames(_layouts(frames, layout, dev), buf[misalign : misalign + need]) == need
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert host[misalign : misalign + need].tobytes() == want
        assert (host[:misalign] == 0xAB).all() and (host[misalign + need :] == 0xAB).all()


# ---------------------------------------------------------------------------------------------------------------- the callback

class _DS:
    def __init__(self, mol, label):
        self.molecule, self._label = mol, label

    def label(self):
        return self._label


class _GpuSampler:
    is_global_zero = True; world_size = 1; global_step = 0

    def __init__(self, dev):
        self.device = dev


def _batch(mols_labels, T, dev, seed, poke=None):
    """Samples as `unbatch_samples` hands them out: [n, T, 3] views of one [T, sum N, 3] device tensor."""
    total = sum(len(m["atom_names"]) for m, _ in mols_labels)
    traj = torch.randn(T, total, 3, generator=torch.Generator().manual_seed(seed))
    if poke is not None:
        poke(traj)
    traj = traj.to(dev)
    out, at = [], 0
    for mol, label in mols_labels:
        n = len(mol["atom_names"])
        out.append({"dataset_label": label, "atom_type_index": mol["atom_type_index"], "xhat_traj": traj[:, at : at + n].permute(1, 0, 2)})
        at += n
    return out


def _trees_equal(a: str, b: str) -> int:
    fa = sorted(os.path.relpath(os.path.join(dp, f), a) for dp, _, fs in os.walk(a) for f in fs)
    fb = sorted(os.path.relpath(os.path.join(dp, f), b) for dp, _, fs in os.walk(b) for f in fs)
    assert fa == fb and fa
    for f in fa:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f
    return len(fa)


def _run_both(tmp_path, batches, datasets, dev, modes=("device", "host"), **kw):
    from jamun_amd.callbacks import SaveTrajectoryCallback

    cbs = {m: SaveTrajectoryCallback(datasets, output_dir=str(tmp_path / m), encode=m, **kw) for m in modes}
    for cb in cbs.values():
        cb.on_sample_start(_GpuSampler(dev))
    for b in batches:
        for cb in cbs.values():
            cb.on_after_sample_batch(b, _GpuSampler(dev))
            cb.flush()
        n_files = _trees_equal(str(tmp_path / modes[0]), str(tmp_path / modes[1]))  # after EVERY batch
    for cb in cbs.values():
        cb.on_sample_end(_GpuSampler(dev))
    return cbs, n_files


@pytest.mark.parametrize("small_staging", [False, True], ids=["staging_default", "staging_64k"])
@pytest.mark.parametrize("restart", [False, True], ids=["running_npy_index", "npy_index_restarts"])
def test_callback_device_tree_equals_host_tree_after_every_batch(tmp_path, monkeypatch, restart, small_staging):
    """Two labels, 4 + 3 chains, 3 batches.  With a 64 KiB staging buffer every file goes through several chunks."""
    from jamun_amd import traj_encode

    if small_staging:
        monkeypatch.setattr(traj_encode, "STAGING_BYTES", 1 << 16)
    dev = _dev()
    a, b = molecule(10), named_chain(29, seed=2)
    walkers = [(a, "a")] * 2 + [(b, "b")] * 3 + [(a, "a")] * 2  # labels interleaved in the batch
    batches = [_batch(walkers, 40, dev, seed=s) for s in range(3)]
    cbs, n_files = _run_both(tmp_path, batches, [_DS(a, "a"), _DS(b, "b")], dev, npy_index_restarts_per_batch=restart)
    n_npy = (4 + 3) if restart else 3 * (4 + 3)
    assert n_files == 2 + 2 * (3 * 7 + 2) + n_npy + 2  # topology.pdb per label; pdb + dcd per chain and joined; npy
    assert len(cbs["device"].chains["a"]) == 12 and len(cbs["device"].chains["b"]) == 9
    assert cbs["device"]._encoder is not None and cbs["host"]._encoder is None
    if small_staging:
        assert cbs["device"]._encoder.staging_bytes() == 3 * (1 << 16)


def test_callback_rewrites_files_with_unencodable_values_on_the_host_path(tmp_path):
    dev = _dev()
    a = molecule(10)
    walkers = [(a, "a")] * 3

    def poke(traj):
        traj[2, 13, 1] = float("nan")  # second chain
        traj[5, 25, 0] = 1000.0        # third chain: 10000.000 Angstrom
        traj[6, 25, 2] = float("inf")

    batches = [_batch(walkers, 9, dev, seed=0), _batch(walkers, 9, dev, seed=1, poke=poke), _batch(walkers, 9, dev, seed=2)]
    _run_both(tmp_path, batches, [_DS(a, "a")], dev)
    txt = open(str(tmp_path / "device" / "a" / "predicted_samples" / "pdb" / "joined.pdb")).read()
    assert "     nan" in txt and "10000.000" in txt and "     inf" in txt


def test_host_batch_then_device_batches_write_the_host_tree(tmp_path):
    """``encode="auto"``: batch 1 arrives as CPU tensors (host path), batches 2 and 3 on the GPU, which extend ``joined.*`` behind files the
    host path wrote; batch 2 carries values no PDB field holds, so its files and ``joined.pdb`` are rewritten by the host formatter."""
    dev = _dev()
    a = molecule(10)
    walkers = [(a, "a")] * 3

    def poke(traj):
        traj[2, 13, 1] = float("nan")
        traj[5, 25, 0] = 1000.0
        traj[6, 25, 2] = float("inf")

    batches = [_batch(walkers, 9, torch.device("cpu"), seed=0), _batch(walkers, 9, dev, seed=1, poke=poke), _batch(walkers, 9, dev, seed=2)]
    cbs, n_files = _run_both(tmp_path, batches, [_DS(a, "a")], dev, modes=("auto", "host"))
    assert n_files == 1 + 3 * (3 * 3 + 1)
    assert cbs["auto"]._encoder is not None and cbs["host"]._encoder is None and not cbs["auto"]._dev_blocks
    txt = open(str(tmp_path / "auto" / "a" / "predicted_samples" / "pdb" / "joined.pdb")).read()
    assert "     nan" in txt and "10000.000" in txt and "     inf" in txt and txt.count("MODEL ") == 3 * 3 * 9


@pytest.mark.parametrize("staging", [case.STAGING_64K, None], ids=["staging_64k", "staging_default"])
def test_all_options_device_tree_has_the_recorded_digests(tmp_path, monkeypatch, golden_dir, staging):
    """_trajectory_device_case.py: superposition, torsions, PDB and DCD of two labels at once.  With 64 KiB of staging a 166-atom chain is
    two aligned spans (32 + 8 frames), each several PDB chunks and one DCD chunk; with the default size everything is one chunk, and the
    bytes are the same: one set of digests, recorded before the writer was split into steps."""
    from jamun_amd import traj_encode

    if staging is not None:
        monkeypatch.setattr(traj_encode, "STAGING_BYTES", staging)
        n = 166
        assert traj_encode.DeviceTrajectoryEncoder.align_frames_per_chunk(n) == traj_encode.DeviceTrajectoryEncoder.dcd_frames_per_chunk(n) == 32
    with open(os.path.join(golden_dir, "trajectory_device_trees.json")) as f:
        want = json.load(f)
    for label in ("m", "c"):  # the recorded set covers every encoded file of both labels
        for ext in ("pdb", "dcd"):
            assert all(f"{label}/predicted_samples/{ext}/{i}.{ext}" in want for i in (list(range(6 if label == "m" else 3)) + ["joined"]))
    got = case.digests(str(tmp_path / "out"), _dev())
    assert sorted(f for f in want if f not in got) == []
    assert sorted(f for f in want if got[f] != want[f]) == []


def test_staging_memory_is_constant(tmp_path):
    """2 000 frames x 16 chains: the encoder's staging memory is the constant, before and after, and device memory does not grow with the
    text (~2.2 MB of PDB per chain here, 36 MB per batch and as much again for the joined file)."""
    from jamun_amd import traj_encode
    from jamun_amd.callbacks import SaveTrajectoryCallback

    dev = _dev()
    mol = molecule(10)
    cb = SaveTrajectoryCallback([_DS(mol, "a")], output_dir=str(tmp_path / "out"), encode="device")
    cb.on_sample_start(_GpuSampler(dev))
    sizes = []
    for s in range(2):
        batch = _batch([(mol, "a")] * 16, 2000, dev, seed=s)
        cb.on_after_sample_batch(batch, _GpuSampler(dev))
        cb.flush()
        sizes.append(cb._encoder.staging_bytes())
        assert cb._encoder._dev.numel() == traj_encode.STAGING_BYTES and [p.numel() for p in cb._encoder._pinned] == [traj_encode.STAGING_BYTES] * 2
    cb.on_sample_end(_GpuSampler(dev))
    assert sizes == [3 * traj_encode.STAGING_BYTES] * 2
    assert not cb._dev_blocks  # the device blocks were released
    joined = str(tmp_path / "out" / "a" / "predicted_samples" / "pdb" / "joined.pdb")
    assert open(joined, "rb").read().count(b"MODEL ") == 2 * 16 * 2000


def test_device_tree_is_written_faster_than_host_tree(tmp_path):
    """Sanity only: 16 chains x 2 000 frames x 17 atoms, all three formats; the measured rates are in profiles/traj_encode_rate.json."""
    from jamun_amd.callbacks import SaveTrajectoryCallback

    dev = _dev()
    mol = named_chain(17, seed=3)
    batch = _batch([(mol, "a")] * 16, 2000, dev, seed=0)
    warm = SaveTrajectoryCallback([_DS(mol, "a")], output_dir=str(tmp_path / "warm"), encode="device")  # library load, stream, pinned memory
    warm.on_after_sample_batch(_batch([(mol, "a")] * 2, 8, dev, seed=1), _GpuSampler(dev))
    warm.on_sample_end(_GpuSampler(dev))
    wall = {}
    for mode in ("device", "host"):
        cb = SaveTrajectoryCallback([_DS(mol, "a")], output_dir=str(tmp_path / mode), encode=mode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cb.on_after_sample_batch(batch, _GpuSampler(dev))
        cb.on_sample_end(_GpuSampler(dev))
        wall[mode] = time.perf_counter() - t0
    print(f"tree of 16 x 2000 x 17: device {wall['device']:.3f} s, host {wall['host']:.3f} s")
    _trees_equal(str(tmp_path / "device"), str(tmp_path / "host"))
    assert wall["device"] < wall["host"], wall
