"""Records tests/golden/trajectory_device_trees.json: the sha256 of every file the run of tests/_trajectory_device_case.py leaves on the device
path with 64 KiB of staging memory.  Recorded on an MI355X from the commit before the writer moved to jamun_amd/trajectory_writer.py;
test_gpu_traj_encode.py holds every later tree to it, so it is not to be recorded again from a tree under test.  Run it TWICE from the
repository root with the library built: the second run keeps only the files whose digest the first one recorded too (and names the
others), so that nothing is pinned that the parent does not reproduce.

    python tests/golden/make_trajectory_device_trees.py

It refuses to record when the default staging size gives other bytes than 64 KiB: the test expects one set of digests for both."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
OUT = os.path.join(HERE, "trajectory_device_trees.json")

if __name__ == "__main__":
    import torch

    import _trajectory_device_case as case
    from jamun_amd import traj_encode

    dev = torch.device("cuda", 0)
    default = traj_encode.STAGING_BYTES
    got = {}
    for name, staging in (("staging_64k", case.STAGING_64K), ("staging_default", default)):
        traj_encode.STAGING_BYTES = staging
        with tempfile.TemporaryDirectory() as root:
            got[name] = case.digests(root, dev)
    traj_encode.STAGING_BYTES = default
    differ = sorted(f for f in got["staging_64k"] if got["staging_default"].get(f) != got["staging_64k"][f])
    if differ or sorted(got["staging_default"]) != sorted(got["staging_64k"]):
        sys.exit(f"the default staging size gives other files than 64 KiB: {differ}")
    files = got["staging_64k"]
    if os.path.exists(OUT):
        with open(OUT) as f:
            before = json.load(f)
        dropped = sorted(f for f in set(files) | set(before) if files.get(f) != before.get(f))
        print(f"second run: {len(dropped)} files differ from the first and are left out: {dropped}")
        files = {f: d for f, d in files.items() if before.get(f) == d}
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(name)}: {json.dumps(d)}" for name, d in files.items()) + "\n}\n")
    print(f"recorded {len(files)} files")
