"""Rate of the trajectory writer, host formatter against device encoder.  Run on the GPU box from the repo root:

    python profiles/tools/traj_encode_rate.py [--frames 400] [--batches 2] [--out profiles/traj_encode_rate.json]

Runs ``SaveTrajectoryCallback`` on cfg2-shaped chains (256 walkers x 17 atoms, WITH atom names, so all three formats are written) once
with ``encode="host"`` (`pdb.save_pdb` / `pdb.save_dcd`, every file rewritten whole) and once with ``encode="device"`` (jamun_traj.hip),
timing ``on_after_sample_batch`` .. ``on_sample_end`` over the batches, and reports frames/s (one frame = one saved (walker, frame) pair —
the unit of bench.py's conformations/s) and MB/s of files written.  Then the device run is repeated in a child process under
``rocprofv3 --kernel-trace --stats`` for the encoder kernels' own time (achieved store rate = bytes the kernels wrote / their summed
duration), and a plain sequential write of page-locked-buffer-sized blocks gives the disk's rate on this machine.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WALKERS, ATOMS = 256, 17


def named_chain(n_atoms):
    from jamun_amd import synth

    mol = synth.random_chain(n_atoms, seed=0)
    els = [["C", "O", "N"][int(t)] for t in mol["atom_type_index"]]
    return dict(mol, atom_names=[(els[i] + ["", "A", "G1", "B"][i % 4])[:4] for i in range(n_atoms)], elements=els,
                residues=[["ALA", "GLY"][(i // 9) % 2] for i in range(n_atoms)], residue_ids=[i // 9 + 1 for i in range(n_atoms)])


class DS:
    def __init__(self, mol):
        self.molecule = mol

    def label(self):
        return "cfg2"


class FakeSampler:
    is_global_zero = True; world_size = 1; global_step = 0

    def __init__(self, dev):
        self.device = dev


def tree_bytes(root):
    return sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(root) for f in fs)


def run_mode(mode, frames, batches, tmp_root):
    import torch

    from jamun_amd.callbacks import SaveTrajectoryCallback

    dev = torch.device("cuda", 0)
    mol = named_chain(ATOMS)
    out = tempfile.mkdtemp(prefix=f"traj_rate_{mode}_", dir=tmp_root)
    cb = SaveTrajectoryCallback([DS(mol)], output_dir=out, encode=mode)
    data = []
    for b in range(batches):
        traj = torch.randn(frames, WALKERS * ATOMS, 3, generator=torch.Generator().manual_seed(b)).to(dev)
        data.append([{"dataset_label": "cfg2", "atom_type_index": mol["atom_type_index"], "xhat_traj": traj[:, w * ATOMS : (w + 1) * ATOMS].permute(1, 0, 2)}
                     for w in range(WALKERS)])
    if mode == "device":  # library load, side stream and staging buffers are paid once per run: not part of the rate
        warm = SaveTrajectoryCallback([DS(mol)], output_dir=os.path.join(out, "warm"), encode=mode)
        warm.on_after_sample_batch([dict(data[0][0], xhat_traj=data[0][0]["xhat_traj"][:, :2])], FakeSampler(dev))
        warm.on_sample_end(FakeSampler(dev))
        shutil.rmtree(os.path.join(out, "warm"))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for batch in data:
        cb.on_after_sample_batch(batch, FakeSampler(dev))
    cb.on_sample_end(FakeSampler(dev))
    wall = time.perf_counter() - t0
    final = tree_bytes(out)
    pdb_bytes = sum(os.path.getsize(p) for p in glob.glob(os.path.join(out, "cfg2", "predicted_samples", "pdb", "*.pdb")))
    dcd_bytes = sum(os.path.getsize(p) for p in glob.glob(os.path.join(out, "cfg2", "predicted_samples", "dcd", "*.dcd")))
    shutil.rmtree(out, ignore_errors=True)
    n_frames = frames * WALKERS * batches
    return {"mode": mode, "wall_s": wall, "frames": n_frames, "frames_per_s": n_frames / wall, "tree_bytes": final, "MB_per_s": final / wall / 1e6,
            "pdb_bytes": pdb_bytes, "dcd_bytes": dcd_bytes, "writer_wait_s": cb.wait_s}


def disk_rate(tmp_root, total=1 << 30, block=32 << 20):
    buf = os.urandom(block)
    path = os.path.join(tmp_root, "traj_rate_disk.bin")
    t0 = time.perf_counter()
    with open(path, "wb") as f:
        for _ in range(total // block):
            f.write(buf)
        t_buffered = time.perf_counter() - t0
        f.flush()
        os.fsync(f.fileno())
    t_synced = time.perf_counter() - t0
    os.unlink(path)
    return {"bytes": total, "block_bytes": block, "buffered_MB_per_s": total / t_buffered / 1e6, "fsync_MB_per_s": total / t_synced / 1e6}


def kernel_stats(frames, batches, tmp_root):
    d = tempfile.mkdtemp(prefix="traj_rate_prof_", dir=tmp_root)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child",
           "--frames", str(frames), "--batches", str(batches), "--tmp", tmp_root]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    out = {"command": "rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/tools/traj_encode_rate.py --child", "returncode": r.returncode}
    child = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not child:
        out["error"] = (r.stderr or r.stdout)[-600:]
        return out
    res = json.loads(child[-1])
    rows = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for k in ("k_encode_pdb", "k_encode_dcd"):
                if k in row["Name"]:
                    rows[k] = {"calls": int(row["Calls"]), "total_ns": int(row["TotalDurationNs"]), "average_ns": float(row["AverageNs"])}
    shutil.rmtree(d, ignore_errors=True)
    # every PDB byte but the END records and every DCD byte behind the 276-byte preambles is one kernel store
    n_pdb_files = n_dcd_files = WALKERS * batches + 1
    stored = {"k_encode_pdb": res["pdb_bytes"] - 4 * n_pdb_files, "k_encode_dcd": res["dcd_bytes"] - 276 * n_dcd_files}
    for k, v in rows.items():
        v["bytes_stored"] = stored[k]
        v["store_GB_per_s"] = stored[k] / v["total_ns"]
    out["kernels"] = rows
    out["wall_s_under_profiler"] = res["wall_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=400)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_encode_rate.json"))
    ap.add_argument("--tmp", default=tempfile.gettempdir())
    ap.add_argument("--child", action="store_true", help="device mode only, one JSON line (the run under rocprofv3)")
    ap.add_argument("--cfg2-conformations-per-s", type=float, default=None, help="bench.py's value on the same machine, copied into the file")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(run_mode("device", a.frames, a.batches, a.tmp)))
        return
    res = {"shape": {"walkers": WALKERS, "atoms": ATOMS, "frames_per_batch": a.frames, "batches": a.batches, "formats": ["npy", "pdb", "dcd"]},
           "host": run_mode("host", a.frames, a.batches, a.tmp), "device": run_mode("device", a.frames, a.batches, a.tmp)}
    res["device_over_host"] = res["device"]["frames_per_s"] / res["host"]["frames_per_s"]
    res["disk"] = disk_rate(a.tmp)
    res["rocprofv3"] = kernel_stats(a.frames, a.batches, a.tmp)
    if a.cfg2_conformations_per_s:
        res["cfg2_walk_conformations_per_s"] = a.cfg2_conformations_per_s
        res["device_writer_over_walk"] = res["device"]["frames_per_s"] / a.cfg2_conformations_per_s
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
