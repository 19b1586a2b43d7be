"""CPU tests of the end-to-end pins (``_cli_cases.py``): the readers, the collation, the config plumbing and the checkpoint loader against
the inputs the oracle consumed (``tests/golden/oracle_cli_*.npz``, fed from ``jamun_amd.synth`` and the files' own bytes), and the proof
that `check_run` can fail: a correct run directory made from the fixture passes, each of six mutations of it is refused."""
import os

import numpy as np
import pytest
import torch

import _cli_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cfg1():
    return cc.load_fixture("oracle_cli_cfg1")


@pytest.fixture(scope="module")
def params():
    return cc.load_fixture("oracle_cli_cfg1_params")


@pytest.fixture(scope="module")
def twoaa():
    return cc.load_fixture("oracle_cli_2aa")


def _assert_reads_as(mol: dict, want: dict, what, pos_ulps: int):
    """A reader's molecule against what the oracle consumed: index tensors equal, bonds as sorted directed-pair sets, positions bit-equal
    (``pos_ulps`` 0) or within that many float32 ulps."""
    for k in cc.INDEX_KEYS:
        assert mol[k].dtype == torch.int32 and np.array_equal(mol[k].numpy(), want[k]), (what, k)
    assert sorted(map(tuple, mol["bonds"].T.tolist())) == want["bonds"], (what, "bonds")
    got = mol["pos"].numpy()
    assert got.dtype == np.float32 and got.shape == want["pos"].shape, (what, got.dtype, got.shape)
    if pos_ulps == 0:
        assert np.array_equal(got, want["pos"]), (what, "pos")
    else:
        assert (np.abs(got.astype(np.float64) - want["pos"].astype(np.float64)) <= pos_ulps * np.spacing(np.abs(want["pos"]))).all(), (what, "pos")


def test_fixtures_are_the_runs_the_tests_drive(cfg1, params, twoaa):
    """Shapes, batch layout and code order of the three fixtures; the clip of the parameter case binds on some atoms and not on others."""
    for fx, T in ((cfg1, 50), (params, 12)):
        assert fx["ptr"].tolist() == [0, 10, 20, 30, 40] and cc.n_batches(fx) == 2
        assert all(fx[f"xhat_traj_{b}"].shape == (T, 40, 3) and fx[f"xhat_traj_{b}"].dtype == np.float32 for b in (0, 1))
        for w in range(1, 4):  # repeat_init_samples: four walkers of one structure
            assert all(np.array_equal(cc.walker_inputs(fx, w)[k], cc.walker_inputs(fx, 0)[k]) for k in ("pos",) + cc.INDEX_KEYS)
    assert 0.0 < float(params["clip_share"]) < 1.0, float(params["clip_share"])
    assert abs(float(params["clip_share"]) - 0.384) < 0.001  # (the share make_oracle_fixtures.py states)
    assert not np.array_equal(cfg1["xhat_traj_0"][:12], params["xhat_traj_0"])
    codes = cc.fixture_codes(twoaa)
    assert codes == sorted(cc.CODES_2AA) and len(codes) == 28
    mols = cc.molecules_2aa()
    assert np.diff(twoaa["ptr"]).tolist() == [mols[c]["pos"].shape[0] for c in codes] and int(twoaa["ptr"][-1]) == 489
    assert all(twoaa[f"xhat_traj_{b}"].shape == (12, 489, 3) for b in (0, 1)) and cc.n_batches(twoaa) == 2
    # equal-sized neighbours exist (what a label exchange would hide behind) and are told apart by the oracle's trajectories
    lab = cc.labels_2aa(twoaa)
    for a, b in (("KR", "RK"), ("FY", "YF"), ("NQ", "QN")):
        sa, sb = (slice(int(twoaa["ptr"][lab[x][0]]), int(twoaa["ptr"][lab[x][1]])) for x in (a, b))
        assert sa.stop - sa.start == sb.stop - sb.start
        assert cc.frame_rmsd(twoaa["xhat_traj_0"][:, sa].transpose(1, 0, 2), twoaa["xhat_traj_0"][:, sb].transpose(1, 0, 2)).min() > 1e3 * cc.RMSD_TOL_NM


def test_pdb_reader_and_collation_give_what_the_oracle_consumed(tmp_path, cfg1):
    """`create_dataset_from_pdbs` on the AG file of the command-line test, then `get_initial_graphs` with repeat_init_samples=4."""
    from jamun_amd import cmdline, pdb

    mol = cc.ag_molecule()
    path = str(tmp_path / "uncapped_AG.pdb")
    pdb.write_pdb(path, mol, mol["pos"][None])
    ds = pdb.create_dataset_from_pdbs([path])
    assert [d.label() for d in ds] == ["uncapped_AG"] and len(ds[0]) == 1
    _assert_reads_as(ds[0][0], cc.walker_inputs(cfg1, 0), "uncapped_AG", pos_ulps=1)  # (decimals of the file -> float32 / 10)
    got = ds[0][0]
    assert got["atom_names"] == mol["atom_names"] and got["residues"] == mol["residues"] and got["residue_ids"] == mol["residue_ids"]
    batch = cmdline.get_initial_graphs(ds, 1, 4)
    assert batch.ptr.tolist() == cfg1["ptr"].tolist() and batch.dataset_label == ["uncapped_AG"] * 4
    for k in cc.INDEX_KEYS:
        assert np.array_equal(batch.as_topology()[k].numpy(), cfg1[k]), k
    assert sorted(map(tuple, batch.bonds.T.tolist())) == sorted(map(tuple, cfg1["bonds"].T.tolist()))
    assert (np.abs(batch.pos.numpy().astype(np.float64) - cfg1["pos"]) <= np.spacing(np.abs(cfg1["pos"]))).all()


def test_directory_reader_and_collation_give_what_the_oracle_consumed(tmp_path, twoaa):
    """`parse_datasets_from_directory` on the 28-code Timewarp tree as the experiment file calls it: datasets sorted by code, per code the
    index tensors and bonds of the real topology, positions = the heavy-atom rows of frame 0 bit for bit; one walker per code collates to
    the fixture's batch."""
    from jamun_amd import cmdline, synth
    from jamun_amd.pdb import parse_datasets_from_directory

    root = tmp_path / "data" / "timewarp" / "2AA-1-large" / "test"
    synth.write_timewarp_tree(str(root), cc.CODES_2AA, n_frames=2)
    kw = dict(root=str(root), traj_pattern="^(.*)-traj-arrays.npz", pdb_pattern="^(.*)-traj-state0.pdb", subsample=1, num_frames=1)
    ds = parse_datasets_from_directory(**kw)
    codes = cc.fixture_codes(twoaa)
    assert [d.label() for d in ds] == codes == sorted(cc.CODES_2AA)
    mols = cc.molecules_2aa()
    for w, d in enumerate(ds):
        assert len(d) == 1
        _assert_reads_as(d[0], cc.walker_inputs(twoaa, w), d.label(), pos_ulps=0)
        assert d[0]["atom_names"] == mols[d.label()]["atom_names"] and d[0]["residues"] == mols[d.label()]["residues"]
        assert d[0]["residue_ids"] == mols[d.label()]["residue_ids"]
    batch = cmdline.get_initial_graphs(ds, 1, 1)
    assert batch.ptr.tolist() == twoaa["ptr"].tolist() and batch.dataset_label == codes
    assert np.array_equal(batch.pos.numpy(), twoaa["pos"])
    for k in cc.INDEX_KEYS:
        assert np.array_equal(batch.as_topology()[k].numpy(), twoaa[k]), k
    assert sorted(map(tuple, batch.bonds.T.tolist())) == sorted(map(tuple, twoaa["bonds"].T.tolist()))
    first = parse_datasets_from_directory(**kw, max_datasets=3)
    assert [d.label() for d in first] == codes[:3]


def test_every_overridden_parameter_reaches_its_own_field(tmp_path):
    """The command line of test_jamun_sample_cfg1_with_every_parameter_overridden composes to an integrator and a batch sampler that hold
    each override in its own field (all are 0.04 or 1.0 in the shipped experiments: a swapped pair would not show there)."""
    from jamun_amd import cmdline
    from jamun_amd import config as C

    cfg = cmdline.compose(["--config-dir=" + os.path.join(ROOT, "configs"), "experiment=sample_custom", "++init_pdbs=[a.pdb]", "++checkpoint_dir=ck",
                           "num_sampling_steps_per_batch=12", "repeat_init_samples=4", "num_batches=2", "++sampler.rng=torch_cpu"] + cc.PARAM_OVERRIDES,
                          cwd=str(tmp_path))
    r = C.resolve(cfg)
    assert r["seed"] == 7 and r["continue_chain"] is True and r["sampler"]["rng"] == "torch_cpu"
    bs = C.instantiate(r["batch_sampler"])
    assert bs.sigma == cc.SIGMA and type(bs.mcmc).__name__ == "BAOAB" and bs.mcmc.steps == 12 and bs.mcmc.save_trajectory is True
    for k, v in cc.PARAM_VALUES.items():
        assert getattr(bs.mcmc, k) == v, k
    assert len(set(cc.PARAM_VALUES.values()) | {cc.SIGMA}) == 6  # pairwise different: no exchange goes unseen


def test_compile_prefixed_checkpoint_file_loads_to_the_same_tensors(tmp_path, monkeypatch):
    """The checkpoint file of the cfg1 run (keys ``g._orig_mod.*``) and the plain one (``g.*``) hand `Denoiser` the same arguments, key by key."""
    from jamun_amd import synth
    from jamun_amd.checkpoint import load_checkpoint_file
    from jamun_amd.model import Denoiser

    seen = []
    monkeypatch.setattr(Denoiser, "__init__", lambda self, state_dict, **kw: seen.append((state_dict, kw)))
    plain = synth.synthetic_state_dict(output_gain=0.05)
    for prefix in ("g._orig_mod.", "g."):
        path = str(tmp_path / f"epoch=7-step=100{len(prefix)}.ckpt")
        torch.save(synth.synthetic_checkpoint(output_gain=0.05, prefix=prefix), path)
        Denoiser.from_checkpoint_dict(load_checkpoint_file(path))
    (sd_a, kw_a), (sd_b, kw_b) = seen
    assert list(sd_a) == list(sd_b) == list(plain)
    for k in plain:
        assert sd_a[k].dtype == plain[k].dtype and torch.equal(sd_a[k], plain[k]) and torch.equal(sd_b[k], plain[k]), k
    assert kw_a == kw_b and kw_a["max_radius"] == 1.0 and kw_a["average_squared_distance"] == 0.332 and kw_a["mean_center"] is True
    assert float(sd_a["output_gain"]) == pytest.approx(0.05)


# ---- the checker can fail ------------------------------------------------------------------------------------------------------------------

def _cfg1_run(tmp_path, fx, name, **hooks):
    run = str(tmp_path / name)
    cc.write_run_from_fixture(run, fx, {"uncapped_AG": (0, 4)}, {"uncapped_AG": cc.ag_molecule()}, **hooks)
    return run, ({"uncapped_AG": (0, 4)}, {"uncapped_AG": cc.ag_molecule()})


def test_checker_accepts_a_correct_run_directory(tmp_path, params, twoaa):
    run, args = _cfg1_run(tmp_path, params, "good")
    assert cc.check_run(run, params, *args) == 0.0
    lab = {c: r for c, r in cc.labels_2aa(twoaa).items() if c in ("KR", "RK", "GG")}
    run2 = str(tmp_path / "good2")
    cc.write_run_from_fixture(run2, twoaa, lab, cc.molecules_2aa())
    report = {}
    assert cc.check_run(run2, twoaa, lab, cc.molecules_2aa(), report) == 0.0 and sorted(report) == ["GG", "KR", "RK"]


def test_checker_refuses_two_equal_sized_labels_exchanged(tmp_path, twoaa):
    """KR and RK have as many atoms as each other: the files of each written from the other's trajectories (its own names, so only numbers tell)."""
    lab = {c: r for c, r in cc.labels_2aa(twoaa).items() if c in ("KR", "RK")}
    mols = cc.molecules_2aa()
    T = twoaa["xhat_traj_0"].shape[0]

    def other(label, chains):
        w = lab["RK" if label == "KR" else "KR"][0]
        a0, a1 = int(twoaa["ptr"][w]), int(twoaa["ptr"][w + 1])
        return [np.ascontiguousarray(np.transpose(twoaa[f"xhat_traj_{b}"][:, a0:a1], (1, 0, 2))) for b in range(2)]

    run = str(tmp_path / "swapped")
    cc.write_run_from_fixture(run, twoaa, lab, mols, chains_of=other)
    assert np.load(os.path.join(run, "sampler", "KR", "predicted_samples", "npy", "0.npy")).shape == (mols["KR"]["pos"].shape[0], T, 3) == (mols["RK"]["pos"].shape[0], T, 3)
    with pytest.raises(AssertionError, match="rmsd"):
        cc.check_run(run, twoaa, lab, mols)
    # ... and whole directories exchanged (names and all) are refused too
    run = str(tmp_path / "swapped_dirs")
    cc.write_run_from_fixture(run, twoaa, lab, mols)
    os.rename(os.path.join(run, "sampler", "KR"), os.path.join(run, "sampler", "tmp"))
    os.rename(os.path.join(run, "sampler", "RK"), os.path.join(run, "sampler", "KR"))
    os.rename(os.path.join(run, "sampler", "tmp"), os.path.join(run, "sampler", "RK"))
    with pytest.raises(AssertionError):
        cc.check_run(run, twoaa, lab, mols)


def test_checker_refuses_frames_first_arrays(tmp_path, params):
    run, args = _cfg1_run(tmp_path, params, "tn3", chains_of=lambda label, chains: [np.ascontiguousarray(np.transpose(c, (1, 0, 2))) for c in chains])
    with pytest.raises(AssertionError):
        cc.check_run(run, params, *args)


def test_checker_refuses_batches_exchanged(tmp_path, params):
    run, args = _cfg1_run(tmp_path, params, "batches", chains_of=lambda label, chains: chains[4:] + chains[:4])
    with pytest.raises(AssertionError, match="rmsd"):
        cc.check_run(run, params, *args)


def test_checker_refuses_joined_in_walker_major_order(tmp_path, params):
    """Chain files right; ``joined`` as w0b0 w0b1 w1b0 ... instead of the chain order b0w0 b0w1 ..."""
    walker_major = lambda label, chains: np.concatenate([chains[4 * b + w] for w in range(4) for b in range(2)], axis=1)
    run, args = _cfg1_run(tmp_path, params, "joined", joined_of=walker_major)
    with pytest.raises(AssertionError, match="joined.npy"):
        cc.check_run(run, params, *args)


def test_checker_refuses_a_dcd_in_nanometres(tmp_path, params):
    run, args = _cfg1_run(tmp_path, params, "nm", frames_for_dcd=lambda frames: frames / np.float32(10.0))  # (save_dcd multiplies by 10)
    with pytest.raises(AssertionError, match="dcd"):
        cc.check_run(run, params, *args)


def test_checker_refuses_one_atom_of_one_frame_off_by_three_tolerances(tmp_path, params):
    """3e-5 nm on one atom of one frame of one chain, all files of the run written consistently from it.  In the frame's RMSD over the
    ten atoms that is 0.95e-5 nm — inside the bar; the checker's per-atom form of the same bar is what refuses it."""
    def nudge(label, chains):
        chains = [c.copy() for c in chains]
        chains[5][3, 7, 1] += np.float32(3e-5)
        return chains

    run, args = _cfg1_run(tmp_path, params, "nudged", chains_of=nudge)
    with pytest.raises(AssertionError, match="one atom"):
        cc.check_run(run, params, *args)
