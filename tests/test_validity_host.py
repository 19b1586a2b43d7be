"""Host tests of jamun_amd/validity.py: the thresholds on the squared distance against float32 sqrt, the numpy specification against a
plainly written loop and against what the reference's own functions counted (tests/golden/validity_reference.npz), the tables' edge
cases, the meter on the host path, and the configuration.  Every comparison is of integers (or of bytes)."""
import importlib.util
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import _validity_cases as vc
from _frames_common import CaseDataset, meter_run, tree
from _traj_molecules import dipeptide, named_chain
from jamun_amd import validity as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _around(center: np.float32, ulps: int) -> np.ndarray:
    """Every float32 within ``ulps`` steps either side of ``center`` (>= 0)."""
    bits = np.array([center], dtype=np.float32).view(np.int32)[0]
    span = np.arange(max(0, int(bits) - ulps), int(bits) + ulps + 1, dtype=np.int64).astype(np.int32)
    return span.view(np.float32)  # (consecutive bit patterns of non-negative floats are consecutive floats)


def _thresholds() -> list:
    rng = np.random.RandomState(5)
    out = rng.uniform(0.05, 0.5, size=150).tolist()
    for tol in (0.0, 0.1, 0.2, 0.35):
        radii = [v for k, v in V.VDW_RADII.items()] + [v for k, v in V.COVALENT_RADII.items()]
        out += [(1 - tol) * (a + b) for a in radii[:7] for b in radii[:7]][::5] + [(1 + tol) * (a + b) for a in radii[7:] for b in radii[7:]][::5]
    out += [float(F32(0.25)), float(F32(0.3)), float(np.nextafter(F32(0.3), F32(1))), 0.5 * (float(F32(0.3)) + float(np.nextafter(F32(0.3), F32(1))))]
    return out


def test_s_below_and_s_above_decide_as_float32_sqrt_does():
    """For random and table-derived thresholds (a float32 and a midpoint of two float32 among them), every float32 s within 300 ulp
    either side of thr**2: fl32(sqrt(s)) < thr <=> s < s_below(thr), fl32(sqrt(s)) > thr <=> s > s_above(thr)."""
    decisions = 0
    for thr in _thresholds():
        s = _around(F32(thr * thr), 300)
        d = np.sqrt(s)
        assert d.dtype == np.float32
        d = d.astype(np.float64)
        lo, hi = V.s_below(thr), V.s_above(thr)
        assert lo.dtype == np.float32 and hi.dtype == np.float32
        assert np.array_equal(d < thr, s < lo), thr
        assert np.array_equal(d > thr, s > hi), thr
        assert (d < thr).any() and (d > thr).any() and not (d < thr).all()
        decisions += 2 * s.size
    assert decisions > 200_000
    for thr in (0.0, -0.0, -0.1, -np.inf):  # no distance is below a threshold <= 0
        assert V.s_below(thr) == 0.0 and V.s_below(thr).dtype == np.float32
    s = _around(F32(0.0), 300)
    assert np.array_equal(np.sqrt(s).astype(np.float64) > 0.0, s > V.s_above(0.0))
    tiny = 1e-30  # (thr**2 is below the float32 range)
    s = _around(F32(0.0), 300)
    assert np.array_equal(np.sqrt(s).astype(np.float64) < tiny, s < V.s_below(tiny)) and np.array_equal(np.sqrt(s).astype(np.float64) > tiny, s > V.s_above(tiny))
    inf = F32(np.inf)
    assert not inf < V.s_below(0.3) and inf > V.s_above(0.3)  # s = +inf: no clash, a bond issue
    with pytest.raises(ValueError):
        V.s_below(float("nan"))
    with pytest.raises(ValueError):
        V.s_above(-1.0)


@pytest.mark.parametrize("case", ["dipeptide", "helix17", "helix all", "chain12"])
def test_counts_host_equals_a_plain_sqrt_and_compare_loop(case):
    if case == "dipeptide":
        mol, tol, frames = dipeptide(), vc.DIPEPTIDE_TOLERANCES, vc.dipeptide_frames(200)[:40]
    elif case == "helix17":
        mol, tol, frames = vc.helix(17), vc.HELIX_TOLERANCES, vc.helix_frames(17, 129)[:24]
    elif case == "helix all":
        mol, tol, frames = vc.helix(7, "all"), vc.HELIX_TOLERANCES, vc.helix_frames(7, 129)[:24]
    else:
        mol, tol = named_chain(12, seed=3), vc.REFERENCE_TOLERANCES
        frames = vc.noisy_frames(mol["pos"].numpy(), 24, seed=12)
    tables = V.validity_tables(mol, *tol)
    counts, bond_frames = V.validity_counts_host(frames, tables)
    want, want_bf, bonds = vc.plain_loop(frames, mol, *tol, V.VDW_RADII, V.COVALENT_RADII)
    assert counts.dtype == np.uint32 and bond_frames.dtype == np.uint32 and counts.shape == (len(frames), 2)
    assert tables["bonds"].tolist() == [list(b) for b in bonds]
    assert np.array_equal(counts, want) and np.array_equal(bond_frames, want_bf)
    assert want.sum(axis=0).min() > 0 or case == "helix all"
    if case in ("dipeptide", "helix17"):
        vc.check_varied(counts)
    # a tensor, a float64 copy (rounded back to float32) and frames with another stride give the same integers
    again = V.validity_counts_host(torch.from_numpy(np.array(frames)), tables)
    wide = V.validity_counts_host(np.array(frames, dtype=np.float64), tables)
    strided = V.validity_counts_host(np.repeat(np.array(frames), 2, axis=0)[::2], tables)
    for c, b in (again, wide, strided):
        assert np.array_equal(c, counts) and np.array_equal(b, bond_frames)


def test_counts_host_with_non_finite_coordinates_and_no_frames():
    mol = vc.helix(6)
    tables = V.validity_tables(mol, *vc.HELIX_TOLERANCES)
    clean = np.array(vc.helix_frames(6, 129)[:8])
    base, _ = V.validity_counts_host(clean, tables)
    for value, bonds_off in ((np.nan, 0), (np.inf, 2), (-np.inf, 2)):
        x = clean.copy()
        x[1, 2, 0] = value  # frame 1 has no noise: clean counts are 0; atom 2 has two bonds
        counts, bond_frames = V.validity_counts_host(x, tables)
        assert base[1].tolist() == [0, 0] and counts[1].tolist() == [0, bonds_off], value
        assert np.array_equal(np.delete(counts, 1, axis=0), np.delete(base, 1, axis=0))
    counts, bond_frames = V.validity_counts_host(clean[:0], tables)
    assert counts.shape == (0, 2) and bond_frames.tolist() == [0] * 5
    with pytest.raises(ValueError):
        V.validity_counts_host(clean[:, :5], tables)
    with pytest.raises(ValueError):
        V.validity_counts_host(clean.astype(np.int32), tables)


def _make_fixtures_module():
    spec = importlib.util.spec_from_file_location("make_validity_fixtures", os.path.join(ROOT, "tests", "golden", "make_validity_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_counts_host_equals_what_the_references_functions_counted():
    """tests/golden/validity_reference.npz holds the issue counts of the reference's _check_volume_exclusion and _check_bond_lengths on
    these very frames (recorded by tests/golden/make_validity_fixtures.py, which also asserts that no distance lies within 4 float32 ulp
    of a threshold), the sulphur case with the reference's own covalent radius 1.005 among them."""
    mk = _make_fixtures_module()
    z = np.load(os.path.join(ROOT, "tests", "golden", "validity_reference.npz"))
    cases = mk.cases()
    assert sorted(k[: -len("_counts")] for k in z.files if k.endswith("_counts")) == sorted(cases)
    for name, (mol, tol, frames) in cases.items():
        tables = V.validity_tables(mol, *tol)
        counts, bond_frames = V.validity_counts_host(frames, tables)
        assert tables["bonds"].tolist() == [list(b) for b in mk.sorted_bonds(mol)]
        assert np.array_equal(counts, z[f"{name}_counts"]), name
        assert np.array_equal(bond_frames, z[f"{name}_bond_frames"]), name
        assert z[f"{name}_counts"].sum(axis=0).min() > 0
    assert int(z["sulphur_bond_frames"][1]) == 200  # CA-S: 0.15 nm against (1 - 0.2) * 1.081: off in every frame


# ---- tables ------------------------------------------------------------------------------------------------------------------------------

def _mol(elements, bonds):
    return {"elements": elements, "bonds": np.array(bonds, dtype=np.int64).reshape(-1, 2).T}


def test_tables_normalise_the_bonds_and_refuse_bad_ones():
    t = V.validity_tables(_mol(["C", "N", "O", "C"], [[2, 1], [0, 1], [1, 2], [3, 0], [0, 1]]), 0.1, 0.2)
    assert t["bonds"].tolist() == [[0, 1], [0, 3], [1, 2]] and t["bonds"].dtype == np.int32
    assert t["num_bonds"] == 3 and t["num_nonbonded_pairs"] == 3 and t["n_atoms"] == 4
    # pairs in row-major order: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); the bonded ones carry 0
    assert t["clash_s"].dtype == np.float32 and (t["clash_s"] == 0).tolist() == [True, False, True, True, False, False]
    assert t["clash_s"][1] == V.s_below(0.9 * (0.170 + 0.152)) and t["clash_s"][4] == V.s_below(0.9 * (0.155 + 0.170))
    assert t["bond_lo_s"].tolist() == [V.s_below(0.8 * (0.076 + 0.071)), V.s_below(0.8 * (0.076 + 0.076)), V.s_below(0.8 * (0.071 + 0.066))]
    assert t["bond_hi_s"].tolist() == [V.s_above(1.2 * (0.076 + 0.071)), V.s_above(1.2 * (0.076 + 0.076)), V.s_above(1.2 * (0.071 + 0.066))]
    torch_bonds = dict(_mol(["C", "N", "O", "C"], [[2, 1]]), bonds=torch.tensor([[2], [1]]))
    assert V.validity_tables(torch_bonds, 0.1, 0.2)["bonds"].tolist() == [[1, 2]]
    for bad in ([[1, 1]], [[0, 4]], [[-1, 2]]):
        with pytest.raises(ValueError, match="bond 0"):
            V.validity_tables(_mol(["C", "N", "O", "C"], bad), 0.1, 0.2)
    with pytest.raises(ValueError, match="elements"):
        V.validity_tables({"bonds": np.zeros((2, 0), dtype=np.int64)}, 0.1, 0.2)
    for tol in ((-0.1, 0.2), (0.1, float("nan")), (float("inf"), 0.2)):
        with pytest.raises(ValueError, match="tolerance"):
            V.validity_tables(_mol(["C", "C"], []), *tol)


def test_tables_radii_other_overrides_and_the_sulphur_default():
    assert V.COVALENT_RADII["S"] == 1.005 and V.VDW_RADII["other"] == 0.150 and V.COVALENT_RADII["other"] == 0.070
    t = V.validity_tables(_mol(["Se", "C", "S"], [[0, 1], [1, 2]]), 0.1, 0.2)  # an element no table knows takes "other"
    assert t["clash_s"][1] == V.s_below(0.9 * (0.150 + 0.180))
    assert t["bond_lo_s"].tolist() == [V.s_below(0.8 * (0.070 + 0.076)), V.s_below(0.8 * (0.076 + 1.005))]
    assert "1.005" in V.validity_tables.__doc__ and "typo" in V.validity_tables.__doc__
    fixed = V.validity_tables(_mol(["Se", "C", "S"], [[0, 1], [1, 2]]), 0.1, 0.2, vdw_radii={"Se": 0.19}, covalent_radii={"S": 0.105, "Se": 0.12})
    assert fixed["clash_s"][1] == V.s_below(0.9 * (0.19 + 0.180)) and fixed["vdw_radii"]["Se"] == 0.19 and fixed["vdw_radii"]["C"] == 0.170
    assert fixed["bond_hi_s"].tolist() == [V.s_above(1.2 * (0.12 + 0.076)), V.s_above(1.2 * (0.076 + 0.105))]
    # Se-C 0.16 nm (inside both ranges), C-S 0.181 nm (far below 0.8 * 1.081, inside 0.181 * (1 +- 0.2)), Se..S 0.24 nm (a clash either way)
    x = np.array([[[0, 0, 0], [0.16, 0, 0], [0.16, 0.181, 0]]], dtype=np.float32)
    assert V.validity_counts_host(x, t)[0].tolist() == [[1, 1]] and V.validity_counts_host(x, fixed)[0].tolist() == [[1, 0]]
    with pytest.raises(ValueError, match="radius"):
        V.validity_tables(_mol(["C"], []), 0.1, 0.2, vdw_radii={"C": -1.0})


def test_a_denominator_of_zero_gives_nan_fractions():
    x = np.array([[[0, 0, 0], [0.15, 0, 0]]], dtype=np.float32)
    t = V.validity_tables(_mol(["C", "C"], [[0, 1]]), 0.1, 0.2)  # its one pair is bonded: nothing can clash
    assert t["num_nonbonded_pairs"] == 0 and t["clash_s"].tolist() == [0.0]
    counts, _ = V.validity_counts_host(x, t)
    vol, bond = V.fractions(counts, t)
    assert counts.tolist() == [[0, 0]] and math.isnan(vol[0]) and bond.tolist() == [0.0] and vol.dtype == np.float64
    t = V.validity_tables(_mol(["C", "C"], []), 0.1, 0.2)  # no bond
    counts, bond_frames = V.validity_counts_host(x, t)
    vol, bond = V.fractions(counts, t)
    assert counts.tolist() == [[1, 0]] and vol.tolist() == [1.0] and math.isnan(bond[0]) and bond_frames.shape == (0,)
    t = V.validity_tables(_mol(["C"], []), 0.1, 0.2)  # one atom
    counts, _ = V.validity_counts_host(x[:, :1], t)
    assert counts.tolist() == [[0, 0]] and t["clash_s"].shape == (0,) and all(math.isnan(v[0]) for v in V.fractions(counts, t))


# ---- the meter on the host path ------------------------------------------------------------------------------------------------------------

def _meter_run(root, batches, mol=None, xyz=None, **kw):
    from jamun_amd.callbacks import ChemicalValidityMetricsCallback

    vtol, btol = vc.DIPEPTIDE_TOLERANCES
    cb, smp = meter_run(ChemicalValidityMetricsCallback, root, mol or dipeptide(), batches, torch.device("cpu"), xyz=xyz,
                        volume_exclusion_tolerance=vtol, bond_length_tolerance=btol, **kw)
    return cb, smp, root / "m" / "chemical_validity"


def _frames_of(sample) -> np.ndarray:
    return np.ascontiguousarray(sample["xhat_traj"].permute(1, 0, 2).numpy())


@pytest.mark.parametrize("T, num, factor", [(60, 100, 1), (100, 100, 1), (350, 100, 3), (350, None, 1), (350, 1000, 1), (350, 7, 50)])
def test_meter_on_cpu_tensors_through_the_callback(tmp_path, T, num, factor):
    """Two batches of two chains; T below, equal to and above num_molecules_per_trajectory, and every frame."""
    from jamun_amd.callbacks import ChemicalValidityMetricsCallback, TrajectoryMetricCallback

    mol = dipeptide()
    batches = vc.chain_batches(mol, torch.device("cpu"), 2, T, 2, seed=60)
    xyz = np.array(vc.dipeptide_frames(300))  # (an array: MDtrajDataset keeps a tensor, both are taken)
    cb, smp, d = _meter_run(tmp_path / "run", batches, xyz=xyz, num_molecules_per_trajectory=num)
    assert isinstance(cb, TrajectoryMetricCallback) and isinstance(cb, ChemicalValidityMetricsCallback)
    assert V.frame_factor(T, num) == factor
    assert sorted(os.listdir(d)) == sorted([f"{i}.npz" for i in range(4)] + ["joined.npz", "tables.json", "true_traj.npz"])
    tables = V.validity_tables(mol, *vc.DIPEPTIDE_TOLERANCES)
    meta = json.load(open(d / "tables.json"))
    assert meta["elements"] == mol["elements"] and meta["bonds"] == tables["bonds"].tolist() and meta["num_bonds"] == 9
    assert meta["num_nonbonded_pairs"] == 36 and meta["volume_exclusion_tolerance"] == 0.35 and meta["bond_length_tolerance"] == 0.2
    assert meta["vdw_radii"] == V.VDW_RADII and meta["covalent_radii"] == V.COVALENT_RADII and meta["num_molecules_per_trajectory"] == num
    keys = ["bond_counts", "bond_frames", "bond_length_issues", "clash_counts", "frame_indices", "volume_exclusion_issues"]

    def expect(frames, offset=0):
        idx = np.arange(0, len(frames), V.frame_factor(len(frames), num))
        counts, bond_frames = V.validity_counts_host(frames[idx], tables)
        return {"frame_indices": idx + offset, "clash_counts": counts[:, 0], "bond_counts": counts[:, 1], "volume_exclusion_issues": counts[:, 0] / 36,
                "bond_length_issues": counts[:, 1] / 9, "bond_frames": bond_frames}

    def same(z, want):
        assert sorted(z.files) == keys
        for k in keys:
            assert np.array_equal(z[k], want[k]), k
        assert z["frame_indices"].dtype == np.int64 and z["clash_counts"].dtype == np.uint32 and z["bond_counts"].dtype == np.uint32
        assert z["volume_exclusion_issues"].dtype == np.float64 and z["bond_length_issues"].dtype == np.float64 and z["bond_frames"].dtype == np.uint32

    same(np.load(d / "true_traj.npz"), expect(xyz))
    chains = [expect(_frames_of(s), offset=i * T) for i, s in enumerate(s for b in batches for s in b)]
    for i, want in enumerate(chains):
        same(np.load(d / f"{i}.npz"), dict(want, frame_indices=want["frame_indices"] - i * T))
        assert len(want["frame_indices"]) == -(-T // factor)
    joined = {k: np.concatenate([c[k] for c in chains]) for k in keys if k != "bond_frames"}
    joined["bond_frames"] = sum(c["bond_frames"] for c in chains)
    same(np.load(d / "joined.npz"), joined)
    if factor == 3 or num is None:
        vc.check_varied(np.stack([joined["clash_counts"], joined["bond_counts"]], axis=1))
    true = {"m/mean_volume_exclusion_issues/true_traj": float(np.mean(expect(xyz)["volume_exclusion_issues"])),
            "m/mean_bond_length_issues/true_traj": float(np.mean(expect(xyz)["bond_length_issues"]))}
    logged = smp.fabric.logged
    assert len(logged) == 2
    for b in range(2):
        want = {}
        for i in (2 * b, 2 * b + 1):
            want[f"m/mean_volume_exclusion_issues/pred_traj_{i}"] = float(np.mean(chains[i]["volume_exclusion_issues"]))
            want[f"m/mean_bond_length_issues/pred_traj_{i}"] = float(np.mean(chains[i]["bond_length_issues"]))
        assert logged[b] == dict(want, **true) and list(logged[b]) == list(want) + list(true)
    # the same run again gives the same bytes
    _, _, d2 = _meter_run(tmp_path / "again", batches, xyz=torch.from_numpy(xyz), num_molecules_per_trajectory=num)
    assert tree(str(d)) == tree(str(d2))


def test_meter_without_dataset_frames_and_its_argument_checks(tmp_path):
    batches = vc.chain_batches(dipeptide(), torch.device("cpu"), 1, 30, 1, seed=61)
    cb, smp, d = _meter_run(tmp_path / "plain", batches)
    assert sorted(os.listdir(d)) == ["0.npz", "joined.npz", "tables.json"]
    assert list(smp.fabric.logged[0]) == ["m/mean_volume_exclusion_issues/pred_traj_0", "m/mean_bond_length_issues/pred_traj_0"]
    with pytest.raises(RuntimeError, match="device='device'"):
        _meter_run(tmp_path / "dev", batches, device="device")  # (CPU tensors)
    with pytest.raises(ValueError, match="device must be"):
        _meter_run(tmp_path / "x", batches, device="gpu")
    with pytest.raises(ValueError, match="num_molecules_per_trajectory"):
        _meter_run(tmp_path / "x", batches, num_molecules_per_trajectory=0)
    no_elements = {k: v for k, v in dipeptide().items() if k != "elements"}
    with pytest.raises(ValueError, match="elements"):
        _meter_run(tmp_path / "x", batches, mol=no_elements)


# ---- configuration -------------------------------------------------------------------------------------------------------------------------

def test_config_names_the_callback_and_the_default_run_does_not():
    from jamun_amd import callbacks, cmdline, config

    cfg_dir = os.path.join(ROOT, "jamun_amd", "hydra_config", "callbacks", "sampler")
    assert "chemical_validity" not in open(os.path.join(cfg_dir, "default.yaml")).read()
    table = next(v for v in vars(config).values() if isinstance(v, dict) and "jamun.callbacks.sampler.SaveTrajectoryCallback" in v)
    assert table["jamun.callbacks.sampler.ChemicalValidityMetricsCallback"] == "jamun_amd.callbacks.ChemicalValidityMetricsCallback"
    base = ["--config-dir=" + os.path.join(ROOT, "configs"), "experiment=sample_custom", "++init_pdbs=[x.pdb]", "++checkpoint_dir=c"]
    assert "chemical_validity" not in cmdline.compose(base)["callbacks"]
    cfg = cmdline.compose(base + ["callbacks=[sampler/default,sampler/chemical_validity]"])["callbacks"]
    assert list(cfg) == ["save_trajectory", "measure_sampling_time", "chemical_validity"]
    entry = cfg["chemical_validity"]
    assert entry["_target_"] == "jamun.callbacks.sampler.ChemicalValidityMetricsCallback"
    assert (entry["bond_length_tolerance"], entry["volume_exclusion_tolerance"], entry["num_molecules_per_trajectory"]) == (0.2, 0.1, 100)
    cb = config.instantiate({k: v for k, v in entry.items() if k != "datasets"}, datasets=[CaseDataset(dipeptide(), "m")])
    assert isinstance(cb, callbacks.ChemicalValidityMetricsCallback)
    meter = cb.meters["m"]
    assert meter.tables["volume_exclusion_tolerance"] == 0.1 and meter.tables["bond_length_tolerance"] == 0.2 and meter.num_molecules_per_trajectory == 100


def test_the_build_names_the_kernel_file_and_native_mirrors_the_header():
    from jamun_amd import _lib, native
    from jamun_amd.csrc import build as b

    assert "jamun_validity.hip" in b.SOURCES and os.path.exists(os.path.join(ROOT, "jamun_amd", "csrc", "jamun_validity.hip"))
    header = open(os.path.join(ROOT, "jamun_amd", "csrc", "jamun_internal.h")).read()
    macro = lambda name: int(re.search(rf"^#define {name} (\d+)", header, flags=re.M).group(1))
    assert native.VALIDITY_MAX_ATOMS == macro("JAMUN_VALIDITY_MAX_ATOMS") >= 256
    assert native.VALIDITY_CHUNK == macro("JAMUN_VALIDITY_CHUNK") and native.VALIDITY_SPLIT_ATOMS == macro("JAMUN_VALIDITY_SPLIT_ATOMS")
    assert "jamun_validity_counts" in _lib.SYMBOLS and hasattr(_lib.load(), "jamun_validity_counts")
    # the wrapper checks its tables before anything needs a GPU
    tables = V.validity_tables(vc.helix(5), *vc.HELIX_TOLERANCES)
    frames = torch.from_numpy(np.array(vc.helix_frames(5, 129)[:4]))
    with pytest.raises(ValueError, match="bond 0"):
        native.validity_counts(frames, dict(tables, bonds=np.array([[0, 5]] * 4, dtype=np.int32)))
    with pytest.raises(ValueError, match="clash_s"):
        native.validity_counts(frames, dict(tables, clash_s=tables["clash_s"][:-1]))
    with pytest.raises(ValueError, match="atoms"):
        native.validity_counts(torch.zeros(1, native.VALIDITY_MAX_ATOMS + 1, 3), tables)
    with pytest.raises(RuntimeError, match="on the GPU"):
        native.validity_counts(frames, tables)  # (valid tables, CPU frames)
