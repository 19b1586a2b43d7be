"""CPU tests: the oracle against the reference-generated golden vectors and analytic known answers."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import denoiser as od
from oracle import e3
from oracle import graph as og
from oracle import walk as ow
from jamun_amd import synth


def _score_fn(d):
    mu = torch.tensor(d["mu"])
    s, a, b = [float(x) for x in d["score_params"]]
    return lambda y: -(y - mu) / (s * s) + a * torch.sin(b * y)


@pytest.mark.parametrize("name", ["baoab_default", "baoab_clip_mass", "baoab_noclip_notraj", "aboba_default", "aboba_clip_mass"])
def test_integrators_match_reference_golden(golden_dir, name):
    d = np.load(os.path.join(golden_dir, name + ".npz"))
    meta = json.load(open(os.path.join(golden_dir, name + ".json")))
    fn = getattr(ow, meta["integrator"])
    noise = ow.RecordedNoise(torch.tensor(d["noise"]))
    y, v, y_traj, score_traj = fn(torch.tensor(d["y0"]), _score_fn(d), noise=noise, **meta["kwargs"])
    # same arithmetic, same order -> bit-exact on CPU
    assert torch.equal(y, torch.tensor(d["y"]))
    assert torch.equal(v, torch.tensor(d["v"]))
    if "y_traj" in d:
        assert torch.equal(y_traj, torch.tensor(d["y_traj"]))
    else:
        assert y_traj is None
    assert torch.equal(score_traj, torch.tensor(d["score_traj"]))


def test_torchnoise_reproduces_recorded_stream(golden_dir):
    d = np.load(os.path.join(golden_dir, "baoab_default.npz"))
    n = ow.TorchNoise(42)
    like = torch.zeros(40, 3)
    for i in range(5):
        assert torch.equal(n(like), torch.tensor(d["noise"][i]))


def test_aboba_without_trajectory_raises_like_reference():
    with pytest.raises(RuntimeError):
        ow.aboba(torch.zeros(4, 3), lambda y: -y, steps=3, noise=ow.TorchNoise(0), save_trajectory=False)


def test_walk_jump_matches_reference_golden(golden_dir):
    d = np.load(os.path.join(golden_dir, "walkjump_baoab.npz"))
    meta = json.load(open(os.path.join(golden_dir, "walkjump_baoab.json")))
    sigma = meta["sigma"]
    sfn = _score_fn(d)
    kw = dict(meta["kwargs"])
    kw.pop("v_init")  # Sampler's v_init="gaussian" overrides the config's "zero" (mcmc/_splitting.py:57)
    out = ow.walk_jump(sfn, lambda y: y + sigma**2 * sfn(y), ow.baoab, torch.tensor(d["y0"]), "gaussian", ow.RecordedNoise(torch.tensor(d["noise"])), **kw)
    for k in ["xhat", "y", "v", "xhat_traj", "y_traj", "score_traj", "sample", "t_traj"]:
        assert torch.equal(out[k], torch.tensor(d[k])), k
    # BAOAB: the jump equals y_t + sigma^2 * score_t
    assert torch.allclose(out["xhat_traj"], out["y_traj"] + sigma**2 * out["score_traj"], atol=1e-6)


def test_encodings_golden(golden_dir):
    enc = json.load(open(os.path.join(golden_dir, "encodings.json")))
    from jamun_amd.data import encode_atom_type, encode_atom_code, encode_residue

    for k, v in enc["atom_type"].items():
        assert encode_atom_type(k) == v
    for k, v in enc["atom_code"].items():
        assert encode_atom_code(k) == v
    for k, v in enc["residue"].items():
        assert encode_residue(k) == v


# ---- e3nn restatement: derived constants and known answers -------------------------------------


def test_wigner_constants():
    assert torch.allclose(e3.wigner_3j(0, 0, 0, torch.float64), torch.ones(1, 1, 1, dtype=torch.float64))
    d = torch.eye(3, dtype=torch.float64) / math.sqrt(3)
    assert torch.allclose(e3.wigner_3j(1, 1, 0, torch.float64)[:, :, 0], d)
    assert torch.allclose(e3.wigner_3j(0, 1, 1, torch.float64)[0], d)
    assert torch.allclose(e3.wigner_3j(1, 0, 1, torch.float64)[:, 0, :], d)
    C = e3.wigner_3j(1, 1, 1, torch.float64)
    eps = torch.zeros(3, 3, 3, dtype=torch.float64)
    for i, j, k in [(0, 1, 2), (1, 2, 0), (2, 0, 1)]:
        eps[i, j, k] = 1
        eps[i, k, j] = -1
    assert torch.allclose(C, eps / math.sqrt(6))


def test_weight_counts_match_reference_shapes():
    hid = e3.parse_irreps("120x0e + 32x1e")
    sh = e3.parse_irreps("1x0e + 1x1e")
    gin = od.gate_in_irreps(hid)
    assert gin == [(152, 0), (32, 1)]
    assert e3.fctp_weight_numel(hid, sh, gin) == 28992
    assert e3.fctp_weight_numel([(8, 0), (8, 0), (32, 0), (8, 0)], sh, gin) == 10304
    assert e3.linear_weight_numel([(8, 0), (8, 0), (32, 0), (8, 0)], hid) == 6720
    assert e3.linear_weight_numel(hid, hid) == 15424
    assert e3.linear_weight_numel(hid, gin) == 19264
    offs = [i[3] for i in e3.fctp_instructions(hid, sh, gin)[0]]
    assert offs == [0, 18240, 22080, 23104, 27968]


def test_normalize2mom_constants():
    assert abs(e3.normalize2mom_const("leaky_relu") - 1.4162684) < 1e-6
    assert abs(e3.normalize2mom_const("sigmoid") - 1.8467055) < 1e-6


def test_fctp_variance_preservation():
    """e3nn's normalisation: unit-variance inputs and weights give ~unit second moment per output component."""
    torch.manual_seed(0)
    hid = e3.parse_irreps("120x0e + 32x1e")
    sh = e3.parse_irreps("1x0e + 1x1e")
    out = [(152, 0), (32, 1)]
    Z = 512
    x = torch.randn(Z, 216)
    v = torch.randn(Z, 3)
    y = e3.spherical_harmonics_01(v)
    w = torch.randn(Z, 28992)
    o = e3.fctp(x, y, w, hid, sh, out)
    assert abs(o[:, :152].pow(2).mean().item() - 1.0) < 0.1
    assert abs(o[:, 152:].pow(2).mean().item() - 1.0) < 0.1
    lin = e3.linear(x, torch.randn(15424), hid, hid)
    assert abs(lin.pow(2).mean().item() - 1.0) < 0.1


def _setup(n_walkers=2, mol=None):
    mol = mol or {k: v for k, v in synth.ag_dipeptide().items() if torch.is_tensor(v)}
    topo = og.collate([mol] * n_walkers)
    return topo


def test_zero_gain_closed_form():
    """output_gain = 0 (reference init, e3conv.py:85) => xhat = mean_center(c_skip * mean_center(y))."""
    topo = _setup()
    sd = synth.synthetic_state_dict(output_gain=0.0)
    hp = od.default_hparams()
    torch.manual_seed(0)
    y = topo["pos"] + 0.04 * torch.randn_like(topo["pos"])
    x = od.xhat(y, topo, 0.04, sd, hp)
    A, B = 0.332, 6 * 0.04**2
    yc = og.mean_center(y, topo["batch"], 2)
    assert torch.allclose(x, og.mean_center(A / (A + B) * yc, topo["batch"], 2), atol=1e-7)


def test_se3_equivariance_and_reflection():
    from scipy.spatial.transform import Rotation

    topo = _setup()
    sd = synth.synthetic_state_dict()
    hp = od.default_hparams()
    torch.manual_seed(0)
    y = (topo["pos"] + 0.04 * torch.randn_like(topo["pos"])).double()
    sd64 = {k: v.double() for k, v in sd.items()}
    x = od.xhat(y, topo, 0.04, sd64, hp)
    R = torch.tensor(Rotation.random(random_state=1).as_matrix())
    x2 = od.xhat(y @ R.T + torch.tensor([0.1, -0.3, 0.2], dtype=torch.float64), topo, 0.04, sd64, hp)
    assert torch.allclose(x2, x @ R.T, atol=1e-10)
    # all irreps are even parity: the 1e x 1e -> 1e (cross product) path breaks reflection equivariance
    x3 = od.xhat(-y, topo, 0.04, sd64, hp)
    assert (x3 + x).abs().max() > 1e-6


def test_radius_graph_cap_and_order():
    torch.manual_seed(0)
    pos = torch.rand(50, 3) * 0.5  # dense: everyone within r
    batch = torch.zeros(50, dtype=torch.long)
    ei = og.radius_graph(pos, 10.0, batch)
    src, dst = ei
    for i in range(50):
        nb = src[dst == i].tolist()
        hits = list(range(50))[:33]
        expect = [j for j in hits if j != i]
        assert nb == expect
    # two graphs never connect
    batch2 = torch.cat([torch.zeros(25), torch.ones(25)]).long()
    ei2 = og.radius_graph(pos, 10.0, batch2)
    assert ((ei2[0] < 25) == (ei2[1] < 25)).all()
    assert ei2.shape[1] == 2 * 25 * 24
    # strict inequality
    p3 = torch.tensor([[0.0, 0, 0], [1.0, 0, 0]])
    assert og.radius_graph(p3, 1.0, torch.zeros(2, dtype=torch.long)).shape[1] == 0


def test_scatter_mean_empty_rows_are_zero():
    src = torch.ones(3, 2)
    out = og.scatter_mean(src, torch.tensor([0, 0, 2]), 4)
    assert torch.equal(out, torch.tensor([[1.0, 1], [0, 0], [1, 1], [0, 0]]))


def test_separable_tensor_product_counts_and_equivariance():
    """SeparableTensorProduct (e3tools/nn/_tensor_product.py:27-47) for the path's irreps: 336 depth-wise weights per edge for
    120x0e + 32x1e (112 for the atom embedding), a point-wise Linear with as many weights as the fully connected product
    (28 992 / 10 304); the product is SO(3)-equivariant and, through the 1e x 1e -> 1e cross product, not reflection-invariant."""
    hid, sh = e3.parse_irreps("120x0e + 32x1e"), e3.parse_irreps("1x0e + 1x1e")
    gate_in = e3.parse_irreps("152x0e + 32x1e")
    emb = e3.parse_irreps("8x0e + 8x0e + 32x0e + 8x0e")
    ins, dtp, numel = e3.separable_instructions(hid, sh, gate_in)
    assert numel == 336 and dtp == [(120, 0), (120, 1), (32, 1), (32, 0), (32, 1)]
    assert e3.linear_weight_numel(dtp, gate_in) == 28992 == e3.fctp_weight_numel(hid, sh, gate_in)
    ins0, dtp0, numel0 = e3.separable_instructions(emb, sh, gate_in)
    assert numel0 == 112 and e3.linear_weight_numel(dtp0, gate_in) == 10304
    torch.manual_seed(0)
    Z = 5
    x = torch.randn(Z, 216, dtype=torch.float64)
    v = torch.randn(Z, 3, dtype=torch.float64)
    w = torch.randn(Z, 336, dtype=torch.float64)
    lw = torch.randn(28992, dtype=torch.float64)
    q, _ = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]

    def rot(feat, n0, n1, R):
        out = feat.clone()
        out[:, n0:] = (feat[:, n0:].reshape(-1, n1, 3) @ R.T).reshape(-1, 3 * n1)
        return out

    f = lambda xx, vv: e3.separable_tp(xx, e3.spherical_harmonics_01(vv), w, lw, hid, sh, gate_in)
    out = f(x, v)
    assert out.shape == (Z, 152 + 96)
    assert (f(rot(x, 120, 32, q), v @ q.T) - rot(out, 152, 32, q)).abs().max() < 1e-10
    P = -torch.eye(3, dtype=torch.float64)  # x1 are 1e (even) vectors: a point reflection of the geometry alone is NOT a symmetry
    assert (f(x, v @ P.T) - out).abs().max() > 1e-3


def test_cached_oracle_fixtures_are_fresh(golden_dir, tmp_path):
    """The GPU tests read cached oracle outputs; re-run a prefix of each kind here and compare bit for bit.  The prefix runs in a child
    process under the generator's PINNED_ENV (one thread, reproducible MKL, generic ATen kernels), the environment the cache was
    written under, so that the bits do not depend on this machine's CPU or thread count."""
    import importlib.util
    import json
    import subprocess
    import sys

    path = os.path.join(golden_dir, "make_oracle_fixtures.py")
    spec = importlib.util.spec_from_file_location("make_oracle_fixtures", path)
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    cases = [
        ("oracle_forward_ag4", {}, ["xhat", "score", "x3", "deg"]),
        ("oracle_forward_sep_ag4", {}, ["xhat", "x2", "deg"]),
        ("oracle_walk_baoab_ag4_50", {"max_steps": 3}, ["xhat_traj", "y_traj"]),
        ("oracle_walk_baoab_ag4_50_mid", {"max_steps": 3}, ["xhat_traj", "y_traj"]),
        ("oracle_walk_aboba_ag4_20", {"max_steps": 3}, ["xhat_traj", "y_traj"]),
        ("oracle_sampler_cc0", {"max_batches": 1}, ["xhat_traj_0"]),
        # the command-line runs (tests/_cli_cases.py): the inputs the oracle read from the files it wrote, and the first frames
        ("oracle_cli_cfg1", {"max_steps": 3, "max_batches": 1}, ["pos", "bonds", "atom_code_index", "xhat_traj_0"]),
        ("oracle_cli_cfg1_params", {"max_steps": 3, "max_batches": 1}, ["xhat_traj_0"]),
        # (489 atoms: half a minute per oracle forward, so the first frame only — the y0 draw over the whole collated batch)
        ("oracle_cli_2aa", {"max_steps": 1, "max_batches": 1}, ["pos", "ptr", "codes", "residue_code_index", "xhat_traj_0"]),
    ]
    code = ("import importlib.util, json, sys\nimport numpy as np, torch\ntorch.set_num_threads(1)\n"
            "spec = importlib.util.spec_from_file_location('mk', sys.argv[1]); mk = importlib.util.module_from_spec(spec); spec.loader.exec_module(mk)\n"
            "out = {}\n"
            "for name, kw, keys in json.loads(sys.argv[3]):\n"
            "    f = mk.CASES[name](**kw)\n"
            "    out.update({name + '__' + k: f[k].numpy() for k in keys})\n"
            "np.savez(sys.argv[2], **out)\n")
    r = subprocess.run([sys.executable, "-c", code, path, str(tmp_path / "fresh.npz"), json.dumps(cases)], env=dict(os.environ, **mk.PINNED_ENV),
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    fresh = np.load(tmp_path / "fresh.npz")
    for name, kw, keys in cases:
        cached = np.load(os.path.join(golden_dir, name + ".npz"))
        for k in keys:
            c = torch.tensor(cached[k])
            f = torch.tensor(fresh[name + "__" + k])
            assert torch.equal(f, c[: f.shape[0]] if f.shape != c.shape else c), (name, k)


def test_fp32_oracle_leaves_fp64_trajectory():
    """Evidence for the trajectory tolerances of tests/test_gpu_parity.py: the walk is a dynamical
    system, and with the strongly non-linear random checkpoint (output gain 0.5) it amplifies fp32 rounding — the fp32
    ORACLE itself leaves the fp64 oracle's trajectory exponentially (about x4 per 5 steps), crossing the 1e-5 nm bar within
    ~20 steps (gain 0.2 behaves the same: 1.5e-5 nm at step 21), so no fp32 implementation can be held to 1e-5 nm at step 50
    there.  With the contractive checkpoints (gains 0.05 and 0.1, used for the 50-step BASELINE configs[0] walks) the same
    comparison stays at 2e-8 .. 7e-8 nm for all 50 frames, which is why the whole-trajectory parity tests use those and the
    chaotic ones are held to the bar on their first frames only."""
    mols = [synth.ag_dipeptide()] * 4
    topo = og.collate([{k: v for k, v in m.items() if torch.is_tensor(v)} for m in mols])
    hp = od.default_hparams()
    sigma, steps = 0.04, 26
    noise = torch.randn(steps + 1, topo["pos"].shape[0], 3, generator=torch.Generator().manual_seed(42))
    kw = dict(steps=steps, delta=0.04, friction=1.0, M=1.0, inverse_temperature=1.0, score_fn_clip=100.0, save_trajectory=True)

    def drift(gain):
        sd = synth.synthetic_state_dict(output_gain=gain)
        res = {}
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            p = {k: v.to(dt) for k, v in sd.items()}
            rec = ow.RecordedNoise(noise)
            pos = topo["pos"].to(dt)
            y0 = pos + rec(pos) * sigma
            _, _, y_traj, score_traj = ow.baoab(y0, lambda y: od.score(y, topo, sigma, p, hp), noise=rec, v_init="gaussian", **kw)
            res[name] = y_traj + sigma**2 * score_traj  # xhat of every frame
        return ((res["f32"].double() - res["f64"]) ** 2).sum(-1).mean(-1).sqrt()  # RMSD per frame, nm

    strong = drift(0.5)
    assert strong[:4].max() < 1e-6                                   # one forward: rounding level (1e-7)
    assert strong[25] > 1e-5                                         # ... but past the parity bar within 25 steps
    growth = (strong[25] / strong[5]).item() ** (1 / 4)               # per 5 steps, over steps 5 -> 25
    assert 2.0 < growth < 8.0, growth
    mid = drift(0.1)
    assert mid.max() < 1e-6, mid.max()                                # contractive: stays at rounding level (measured 7e-8)


# ---- pin kit (tests/golden/make_reference_fixtures.py): the oracle against fixtures produced by the reference's OWN classes -----------
def _load_generator(golden_dir, name):
    import importlib.util

    spec = importlib.util.spec_from_file_location(name, os.path.join(golden_dir, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference_case_inputs(golden_dir, name):
    """(molecules, checkpoint, sigma) of `reference_forward_<name>.npz` — the mapping of make_reference_fixtures.FORWARD_CASES, restated
    here because that script cannot be imported without the third-party wheels it exists to call."""
    mk = _load_generator(golden_dir, "make_oracle_fixtures")
    cases = {"ag4": ("ag4", None), "chain17x6": ("chain17x6", None), "ragged": ("ragged", None), "chig93x2": ("chig93x2", None),
             "dipep48": ("dipep48", None), "sep_ag4": ("ag4", "sep"), "trained_ragged": ("ragged", "trained"), "nl2_ragged": ("ragged", "nl2")}
    kind, variant = cases[name]
    if variant == "sep":
        ck, sigma = synth.synthetic_checkpoint(output_gain=mk.GAINS["strong"], separable=True), mk.SIGMA
    elif variant is not None:
        ck, sigma = mk.variant_checkpoint(variant), mk.VARIANTS[variant]["sigma"]
    else:
        ck, sigma = synth.synthetic_checkpoint(output_gain=mk.GAINS["strong"]), mk.SIGMA
    return mk, mk.molecules(kind), ck, sigma


def test_reference_pin_kit_reaches_the_third_party_line(golden_dir):
    """In this image the pin kit must stop at `import e3nn` — not earlier (a typo, a missing generator) and not at another module: the
    import graph and every statement up to the third-party line are exercised.  With e3nn installed the test checks nothing."""
    import importlib.util
    import subprocess
    import sys

    if importlib.util.find_spec("e3nn") is not None:
        pytest.skip("e3nn is installed: run tests/golden/make_reference_fixtures.py and let the fixture tests below judge")
    r = subprocess.run([sys.executable, os.path.join(golden_dir, "make_reference_fixtures.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert r.stderr.strip().splitlines()[-1] == "ModuleNotFoundError: No module named 'e3nn'", r.stderr[-2000:]
    assert "import_reference" in r.stderr and "jamun_amd" not in r.stderr.split("import_reference")[-1]


def test_oracle_matches_reference_fixtures(golden_dir, monkeypatch):
    """`oracle/` against `reference_*.npz` (outputs of jamun.model.Denoiser / e3nn / torch_cluster / torch_scatter themselves).  Skips
    while the fixtures do not exist — they cannot be generated in an image without e3nn; DESIGN.md section 5 says 'parity unpinned'
    until this test has run."""
    import glob

    files = sorted(glob.glob(os.path.join(golden_dir, "reference_forward_*.npz")))
    ops_file = os.path.join(golden_dir, "reference_ops.npz")
    if not files and not os.path.exists(ops_file):
        pytest.skip("no tests/golden/reference_*.npz: generate with tests/golden/make_reference_fixtures.py where e3nn 0.5.4 / torch_cluster / torch_scatter exist")
    if os.path.exists(ops_file):
        d = {k: (torch.tensor(v) if v.dtype.kind in "fiu" else v) for k, v in np.load(ops_file).items()}
        assert torch.allclose(e3.spherical_harmonics_01(d["sh_in"]), d["sh_out"], atol=1e-6)
        assert torch.allclose(e3.soft_one_hot_linspace_gaussian(d["rbf_in"], 0.0, 0.58726, 32), d["rbf_out"], atol=1e-6)
        for key in [k for k in d if k.startswith("w3j_")]:
            l1, l2, l3 = (int(c) for c in key[4:])
            assert torch.allclose(e3.wigner_3j(l1, l2, l3), d[key].float(), atol=1e-6), key  # (incl. the SIGN of (1,1,1))
        for tag, i1, io in (("hidden", "120x0e + 32x1e", "152x0e + 32x1e"), ("init", "8x0e + 8x0e + 32x0e + 8x0e", "152x0e + 32x1e"), ("small", "3x0e + 2x1e", "4x0e + 3x1e")):
            got = e3.fctp(d[f"fctp_{tag}_x1"], d[f"fctp_{tag}_x2"], d[f"fctp_{tag}_w"], e3.parse_irreps(i1), e3.parse_irreps("1x0e + 1x1e"), e3.parse_irreps(io))
            assert torch.allclose(got, d[f"fctp_{tag}_out"], rtol=1e-5, atol=1e-5), tag
        for tag, ii, io in (("self", "120x0e + 32x1e", "120x0e + 32x1e"), ("skip0", "8x0e + 8x0e + 32x0e + 8x0e", "120x0e + 32x1e"),
                            ("head", "120x0e + 32x1e", "152x0e + 32x1e"), ("out", "120x0e + 32x1e", "1x1e")):
            got = e3.linear(d[f"linear_{tag}_x"], d[f"linear_{tag}_w"], e3.parse_irreps(ii), e3.parse_irreps(io))
            assert torch.allclose(got, d[f"linear_{tag}_out"], rtol=1e-5, atol=1e-5), tag
        assert torch.allclose(e3.gate(d["gate_x"], 120, 32), d["gate_out"], rtol=1e-5, atol=1e-6)
        assert abs(e3.normalize2mom_const("leaky_relu") - float(d["n2m_leaky_relu"])) < 1e-6
        assert abs(e3.normalize2mom_const("sigmoid") - float(d["n2m_sigmoid"])) < 1e-6
        assert torch.allclose(og.scatter_mean(d["scatter_src"], d["scatter_index"], 11), d["scatter_mean"], atol=1e-6)
        if "rg_cuda" in d:  # index-order rule: the oracle's (and the HIP path's) semantics
            mine = og.radius_graph(d["rg_pos"], float(d["rg_r"]), torch.zeros(48, dtype=torch.long))
            assert set(map(tuple, mine.t().tolist())) == set(map(tuple, d["rg_cuda"].t().tolist()))
        # CPU rule: same neighbour COUNT per centre; which 32 of the candidates is kd-tree order (not restated: oracle/graph.py:25-26)
        mine = og.radius_graph(d["rg_pos"], float(d["rg_r"]), torch.zeros(48, dtype=torch.long))
        assert torch.equal(torch.bincount(mine[1], minlength=48), torch.bincount(d["rg_cpu"][1], minlength=48))
    for f in files:
        name = os.path.basename(f)[len("reference_forward_"):-len(".npz")]
        cuda = name.endswith("_cuda")
        mk, mols, ck, sigma = _reference_case_inputs(golden_dir, name[:-5] if cuda else name)
        ref = {k: (torch.tensor(v) if v.dtype.kind in "fiu" else v) for k, v in np.load(f).items()}
        topo = og.collate([{k: v for k, v in m.items() if torch.is_tensor(v)} for m in mols])
        p = {k[2:]: v for k, v in ck["state_dict"].items()}
        hp = mk.variant_hparams(ck)
        # the reference's own edge list drives the oracle's network (its CPU radius graph keeps other neighbours than index order above the
        # cap); where no atom is at the cap the oracle's own edge list must be the same SET
        mine_ei, mine_bm = od.add_edges(og.mean_center(ref["y"], topo["batch"], topo["num_graphs"]), topo, _cutoff(sigma, hp))
        if int(ref["deg"].max()) < 32 + int(torch.bincount(topo["bonds"][1], minlength=ref["y"].shape[0]).max()):
            assert set(map(tuple, torch.cat((mine_ei, mine_bm[None])).t().tolist())) == set(map(tuple, torch.cat((ref["edge_index"], ref["bond_mask"][None])).t().tolist())), name
        monkeypatch.setattr(od, "add_edges", lambda pos, topo_, cut, _e=ref["edge_index"], _b=ref["bond_mask"]: (_e, _b))
        x, inter = od.xhat(ref["y"], topo, sigma, p, hp, return_intermediates=True)
        for l in range(hp["n_layers"] + 1):
            r = ref[f"x{l}"]
            assert (inter[f"x{l}"] - r).abs().max().item() <= 2e-5 * max(r.abs().max().item(), 1e-6), (name, l)
        assert (inter["g"] - ref["g"]).abs().max().item() <= 2e-5 * max(ref["g"].abs().max().item(), 1.0), name
        rm = ((x.double() - ref["xhat"].double()) ** 2).sum(-1).mean().sqrt().item()
        assert rm <= 1e-5, (name, rm)  # north_star's bar: 1e-4 Angstrom
        monkeypatch.undo()


def _cutoff(sigma, hp):
    sig = torch.as_tensor(sigma, dtype=torch.float32)
    c_in = od.normalization_factors(sig, hp["average_squared_distance"])[0]
    return torch.sqrt(torch.as_tensor(hp["max_radius"] ** 2, dtype=torch.float32) + 6 * sig**2) / c_in


# ---- how much does the neighbour-cap RULE matter?  (model/denoiser.py:149) ---------------------------------------
def _capped_graph(pos, r, batch, rule, seed=0):
    """Radius graph with the 32-neighbour cap applied by three rules: "index" = torch_cluster CUDA (first 33 hits incl. self in index order;
    the oracle's and the HIP path's rule), "nearest" = the 32 nearest, "random" = first 33 hits of a random visiting order (a stand-in
    for torch_cluster's CPU kd-tree order, which is neither index order nor nearest-first)."""
    N = pos.shape[0]
    g = torch.Generator().manual_seed(seed)
    src, dst = [], []
    for i in range(N):
        same = (batch == batch[i]).nonzero().flatten()
        d2 = ((pos[same] - pos[i]) ** 2).sum(-1)
        hit = same[d2 < r * r]
        if rule == "index":
            keep = hit[:33]
        elif rule == "nearest":
            order = torch.argsort(((pos[hit] - pos[i]) ** 2).sum(-1), stable=True)
            keep = hit[order[:33]].sort().values  # (self is the nearest: 33 incl. self = 32 neighbours)
        else:
            keep = hit[torch.randperm(hit.numel(), generator=g)[:33]].sort().values
        for j in keep.tolist():
            if j != i:
                src.append(j)
                dst.append(i)
    return torch.tensor([src, dst], dtype=torch.long).reshape(2, -1)


@pytest.mark.parametrize("kind", ["chig166", "dense70"])
def test_sensitivity_of_xhat_to_the_neighbour_cap_rule(kind, monkeypatch):
    """configs[4] asks for an RMSD check "vs CPU"; torch_cluster's CPU build keeps other neighbours than its CUDA build once an atom has
    more than 32 inside the cutoff.  This path implements the CUDA rule.  Measured here, on the bench checkpoint: how
    far apart x-hat is between cap rules — orders of magnitude above the 1e-5 nm parity bar, i.e. on capped molecules the reference's
    own two devices do not agree with each other to the bar, and parity can only be defined against ONE of them."""
    mol = synth.random_chain(166, seed=5) if kind == "chig166" else synth.random_chain(70, seed=3, bond=0.12, min_dist=0.13)
    topo = og.collate([{k: v for k, v in mol.items() if torch.is_tensor(v)}])
    ck = synth.synthetic_checkpoint()
    p = {k[2:]: v for k, v in ck["state_dict"].items()}
    hp = od.default_hparams()
    sigma = 0.04
    torch.manual_seed(2)
    y = topo["pos"] + sigma * torch.randn_like(topo["pos"])
    out, capped = {}, None
    for rule in ("index", "nearest", "random"):
        monkeypatch.setattr(od, "radius_graph", lambda pos, r, batch, _rule=rule: _capped_graph(pos, float(r), batch, _rule))
        x, inter = od.xhat(y, topo, sigma, p, hp, return_intermediates=True)
        out[rule] = x
        if rule == "index":
            rad_deg = torch.bincount(inter["edge_index"][1][inter["bond_mask"] == 0], minlength=y.shape[0])
            capped = (rad_deg >= 32).float().mean().item()
            assert torch.equal(inter["edge_index"][:, inter["bond_mask"] == 0], og.radius_graph(inter["y_centered"], float(_cutoff(sigma, hp)), topo["batch"]))
    rm = lambda a, b: ((a.double() - b.double()) ** 2).sum(-1).mean().sqrt().item()
    r_near, r_rand = rm(out["index"], out["nearest"]), rm(out["index"], out["random"])
    print(f"\n[cap rule] {kind}: {capped:.0%} of atoms at the cap; RMSD(x-hat) index vs nearest {r_near:.3e} nm, index vs random order {r_rand:.3e} nm")
    assert capped > 0.05  # the cap binds on this molecule
    assert r_near > 1e-4 and r_rand > 1e-4  # >= 10 x the parity bar: the rule is not a rounding-level choice
