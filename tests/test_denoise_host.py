"""CPU tests of the denoising evaluation: the host mirrors of ``jamun_amd.native_denoise`` against the fp64 restatement of
_denoise_cases.py, the premises test_gpu_denoise.py rests on (which cases have a well-conditioned rotation and which have none), the
refusals of the binding and of the two C entries that need no GPU, the normalisation factors against the oracle's, and the files of
``denoise_eval.evaluate_denoiser`` with a stub model."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import _denoise_cases as dc
from _denoise_cases import RMSD_TOL_NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0**-24  # unit roundoff of float32


def _names(kind):
    return dc.batch(kind)[3]


# ------------------------------------------------------------------------------------------------------------------ premises of the GPU file

@pytest.mark.parametrize("sigma", dc.SIGMAS)
@pytest.mark.parametrize("kind", list(dc.BATCHES))
def test_non_degenerate_graphs_sit_above_the_gap_floor_and_degenerate_ones_have_no_gap(kind, sigma):
    for mean_center in (True, False):
        _, _, _, _, gap = dc.aligned_case(kind, sigma, mean_center)
        for name, g in zip(_names(kind), gap):
            if name in dc.DEGENERATE:
                assert g <= 1e-6, (name, g)  # one atom, two atoms, a line: the top eigenvalue is (numerically) double
            else:
                assert g >= dc.G_FLOOR, (name, g)
    print(f"{kind} sigma {sigma}: smallest gap of a non-degenerate graph {min(g for n, g in zip(_names(kind), gap) if n not in dc.DEGENERATE):.3f}")


@pytest.mark.parametrize("which", list(dc.SPECIAL_SIGNS))
def test_special_inputs_are_what_they_claim(which):
    x, noise, ptr, y0 = dc.special_case(which)
    assert (dc.horn_gap(y0, x, ptr) >= dc.G_FLOOR).all()
    rm = dc.graph_rmsd(dc.kabsch_reference(y0, x, ptr), x, ptr)
    if which == "mirror":  # chiral molecules: the mirror image does not come back
        assert rm.min() > 100 * RMSD_TOL_NM
    else:
        assert rm.max() < 1e-12


# ------------------------------------------------------------------------------------------------ the host mirrors against the restatement

@pytest.mark.parametrize("sigma", dc.SIGMAS)
@pytest.mark.parametrize("kind", list(dc.BATCHES))
def test_noise_align_host_against_the_fp64_restatement(kind, sigma):
    from jamun_amd import native_denoise as nd

    x, noise, ptr, names = dc.batch(kind)
    x_c, y0, y_ref, rmsd_ref, _ = dc.aligned_case(kind, sigma)
    hx, hy, hr = nd.noise_align_graphs_host(x, noise, ptr, sigma)
    assert np.array_equal(hx, x_c) and hx.dtype == hy.dtype == hr.dtype == np.float32
    # the centring in float64 from the same inputs: the fp32 steps stay within a few ulp of the largest coordinate (|x| < 4 nm)
    s32 = float(np.float32(sigma))
    for g, lo, hi in dc.graphs(ptr):
        xc64 = x[lo:hi].astype(np.float64) - x[lo:hi].astype(np.float64).mean(axis=0)
        y64 = xc64 + s32 * noise[lo:hi].astype(np.float64)
        y64 -= y64.mean(axis=0)
        assert np.abs(hx[lo:hi] - xc64).max() <= 8 * U * 4.0 and np.abs(y0[lo:hi] - y64).max() <= 16 * U * 4.0
    dev = dc.graph_rmsd(hy, y_ref, ptr)
    for name, d in zip(names, dev):
        if name not in dc.DEGENERATE:
            assert d <= 4 * U * 4.0, (name, d)  # the float32 store of the float64 result
    assert np.abs(hr.astype(np.float64) - rmsd_ref).max() <= 1e-7
    assert np.isfinite(hy).all()


def test_host_mirror_switches_and_empty_graphs():
    from jamun_amd import native_denoise as nd

    x, noise, ptr, _ = dc.batch("ragged")
    f = np.float32
    x_c, y, r = nd.noise_align_graphs_host(x, noise, ptr, 0.4, mean_center=False, align=False)
    assert np.array_equal(x_c, x) and np.array_equal(y, x + f(0.4) * noise)
    # a graph without atoms in the middle and at the end
    ptr2 = np.array([0, 10, 10, x.shape[0], x.shape[0]], dtype=np.int32)
    x_c, y, r = nd.noise_align_graphs_host(x, noise, ptr2, 0.4)
    assert r[1] == 0 and r[3] == 0 and np.isfinite(y).all()
    out = nd.denoise_loss_host(y, x_c, ptr2, 0.4, 2.0)
    assert not out[1].any() and not out[3].any() and (out[0] > 0).all()


@pytest.mark.parametrize("sigma", dc.SIGMAS)
@pytest.mark.parametrize("kind", list(dc.BATCHES))
def test_denoise_loss_host_within_the_bound_of_a_sequential_sum(kind, sigma):
    """(n + 4) 2^-24 relative: a sequential fp32 sum of n non-negative terms plus the per-term roundings."""
    from jamun_amd import native_denoise as nd

    _, _, ptr, _ = dc.batch(kind)
    x_c, y0, *_ = dc.aligned_case(kind, sigma)
    W = len(ptr) - 1
    lw = (1.0 + np.arange(W) / W).astype(np.float32)
    inv = float(np.float32(7.25))
    ref = dc.loss_reference(y0, x_c, ptr, sigma, lw, inv)
    got = nd.denoise_loss_host(y0, x_c, ptr, sigma, inv, lw)
    n = np.diff(ptr)[:, None]
    rel = np.abs(got - ref) / np.where(ref > 0, ref, 1.0)
    print(f"{kind} sigma {sigma}: worst error over bound {(rel / ((n + 4) * U)).max():.3f}")
    assert (rel <= (n + 4) * U).all()
    ones = nd.denoise_loss_host(y0, x_c, ptr, sigma, inv, np.ones(W, dtype=np.float32))
    assert np.array_equal(nd.denoise_loss_host(y0, x_c, ptr, sigma, inv), ones)


def test_cpu_tensors_take_the_host_mirror_and_w0_is_empty():
    from jamun_amd import native

    x, noise, ptr, _ = dc.batch("ragged")
    tx, tn, tp = torch.from_numpy(x.copy()), torch.from_numpy(noise.copy()), torch.from_numpy(ptr.copy())
    hx, hy, hr = native.noise_align_graphs_host(x, noise, ptr, 0.04)
    out_y = torch.empty_like(tx)
    gx, gy, gr = native.noise_align_graphs(tx, tn, tp, 0.04, out_y=out_y)
    assert gy is out_y and np.array_equal(gx.numpy(), hx) and np.array_equal(gy.numpy(), hy) and np.array_equal(gr.numpy(), hr)
    loss = native.denoise_loss(gy, gx, tp.long(), 0.04, 3.0)
    assert loss.shape == (len(ptr) - 1, 3) and np.array_equal(loss.numpy(), native.denoise_loss_host(hy, hx, ptr, 0.04, 3.0))
    e = torch.empty(0, 3)
    ex, ey, er = native.noise_align_graphs(e, e, torch.zeros(1, dtype=torch.int64), 0.04)
    assert ex.shape == ey.shape == (0, 3) and er.shape == (0,)
    assert native.denoise_loss(e, e, [0], 0.04, 1.0).shape == (0, 3)


# ------------------------------------------------------------------------------------------------------------------------------ refusals

def _good():
    x, noise, ptr, _ = dc.batch("ragged")
    return dict(x=torch.from_numpy(x.copy()), noise=torch.from_numpy(noise.copy()), ptr=torch.from_numpy(ptr.copy()), sigma=0.04)


REFUSALS = [
    ("x", lambda a: a.update(x=a["x"].double()), "x must be float32"),
    ("x", lambda a: a.update(x=a["x"].reshape(-1)), r"x must be \[N, 3\]"),
    ("x", lambda a: a.update(x=a["x"].numpy()), "x must be a tensor"),
    ("noise", lambda a: a.update(noise=a["noise"][:-1]), r"noise must be \["),
    ("noise", lambda a: a.update(noise=a["noise"].half()), "noise must be float32"),
    ("noise", lambda a: a.update(noise=a["noise"].t().contiguous().t()), "noise must be contiguous"),
    ("noise", lambda a: a.update(noise=a["noise"].to("meta")), "noise must be on cpu like x"),
    ("ptr", lambda a: a.update(ptr=a["ptr"][:-1]), "ptr must run from 0 to N"),
    ("ptr", lambda a: a.update(ptr=a["ptr"] + 1), "ptr must run from 0 to N"),
    ("ptr", lambda a: a.update(ptr=torch.tensor([0, 20, 10, a["x"].shape[0]])), "ptr must be monotone"),
    ("ptr", lambda a: a.update(ptr=a["ptr"].float()), "ptr must hold integers"),
    ("ptr", lambda a: a.update(ptr=a["ptr"].reshape(1, -1)), r"ptr must be \[W \+ 1\]"),
    ("sigma", lambda a: a.update(sigma=0.0), "sigma must be finite and above 0"),
    ("sigma", lambda a: a.update(sigma=-0.04), "sigma must be finite and above 0"),
    ("sigma", lambda a: a.update(sigma=float("nan")), "sigma must be finite and above 0"),
    ("sigma", lambda a: a.update(sigma=float("inf")), "sigma must be finite and above 0"),
]


@pytest.mark.parametrize("name,edit,text", REFUSALS, ids=[f"{n}-{i}" for i, (n, _, _) in enumerate(REFUSALS)])
def test_the_binding_refuses_by_argument_name_before_any_gpu_call(name, edit, text):
    from jamun_amd import native

    a = _good()
    edit(a)
    with pytest.raises(RuntimeError, match=text):
        native.noise_align_graphs(a["x"], a["noise"], a["ptr"], a["sigma"])
    b = dict(a, xhat=a["noise"]) if name == "noise" else dict(a, xhat=_good()["noise"])
    with pytest.raises(RuntimeError, match=text.replace("noise", "xhat")):
        native.denoise_loss(b["xhat"], b["x"], b["ptr"], b["sigma"], 1.0)


def test_the_binding_refuses_bad_result_buffers_and_weights():
    from jamun_amd import native

    a = _good()
    W = a["ptr"].numel() - 1
    for kw, text in ((dict(out_x=torch.empty(3, 3)), "out_x must be"), (dict(out_y=torch.empty_like(a["x"]).double()), "out_y must be"),
                     (dict(rmsd=torch.empty(W + 1)), "rmsd must be")):
        with pytest.raises(RuntimeError, match=text):
            native.noise_align_graphs(a["x"], a["noise"], a["ptr"], a["sigma"], **kw)
    for kw, text in ((dict(loss_weight=torch.ones(W + 1)), "loss_weight must be"), (dict(loss_weight=torch.ones(W).double()), "loss_weight must be"),
                     (dict(out=torch.empty(W, 2)), "out must be")):
        with pytest.raises(RuntimeError, match=text):
            native.denoise_loss(a["noise"], a["x"], a["ptr"], a["sigma"], 1.0, **kw)
    with pytest.raises(RuntimeError, match="inv_c_out_sq must be finite"):
        native.denoise_loss(a["noise"], a["x"], a["ptr"], a["sigma"], float("inf"))


def test_c_entries_refuse_without_a_gpu():
    """Null pointers, negative counts, sigma that is not positive and finite and sizes beyond 31 bits end before any HIP call; n_graphs = 0
    launches nothing and succeeds."""
    from jamun_amd import _lib

    lib = _lib.load()
    host = C.create_string_buffer(64)
    h = C.addressof(host)
    f = C.c_float

    def na(x=h, noise=h, ptr=h, W=1, N=1, sigma=0.04, xc=h, y=h):
        code = lib.jamun_noise_align_graphs(x, noise, ptr, W, N, f(sigma), 1, 1, xc, y, None, None)
        return code, lib.jamun_last_error().decode()

    def dl(xhat=h, x=h, ptr=h, W=1, N=1, sigma=0.04, out=h):
        code = lib.jamun_denoise_loss(xhat, x, ptr, W, N, f(sigma), None, f(1.0), out, None)
        return code, lib.jamun_last_error().decode()

    for call in (na, dl):
        for kw in ({"x": None}, {"ptr": None}, {"y": None} if call is na else {"out": None}):
            assert call(**kw) == (-1, "null argument"), kw
        for kw in ({"W": -1}, {"N": -1}):
            assert call(**kw) == (-1, "negative argument"), kw
        for s in (0.0, -1.0, float("nan"), float("inf")):
            code, text = call(sigma=s)
            assert code == -1 and "must be finite and above 0" in text, s
        code, text = call(N=2**31 - 1)
        assert code == -1 and "must fit 31 bits" in text
        assert call(W=2**31 - 1)[0] == -1
        assert call(W=0, N=0)[0] == 0


# -------------------------------------------------------------------------------------------------------------------- Denoiser, ABI, driver

@pytest.mark.parametrize("sigma", [0.01, 0.04, 0.4, 1.0])
def test_normalization_factors_and_loss_weight_are_the_oracles(sigma):
    from jamun_amd.model import Denoiser
    from oracle import denoiser as od

    mine = Denoiser.normalization_factors(sigma, 0.332)
    ref = od.normalization_factors(sigma, 0.332)
    for a, b in zip(mine, ref):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    assert torch.equal(Denoiser.loss_weight(sigma, 0.332), 1 / (ref[2] ** 2))
    c_out64 = od.normalization_factors(sigma, 0.332, dtype=torch.float64)[2]
    assert abs(float(Denoiser.loss_weight(sigma, 0.332)) * float(c_out64) ** 2 - 1.0) < 1e-6


def test_header_and_binding_table_carry_both_entries():
    from jamun_amd import _lib, native
    from jamun_amd.csrc import build as b

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jamun_hip.h")).read(), flags=re.S)
    for name in ("jamun_noise_align_graphs", "jamun_denoise_loss"):
        assert re.search(rf"\bint {name}\s*\(", hdr) and name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    assert "jamun_denoise.hip" in b.SOURCES and "jamun_denoise.cpp" in b.SOURCES and _lib.ABI_VERSION == 6
    assert native.noise_align_graphs.__module__ == native.denoise_loss.__module__ == "jamun_amd.native_denoise"
    # the two sources share a stem: their cached objects must not
    assert len({os.path.basename(p).split(".")[0] + os.path.splitext(s)[1] for s in b.SOURCES for p in [s]}) == len(b.SOURCES)


class _StubModel:
    """``noise_and_denoise`` returns the centred x moved by ``offset_nm`` in every component (up for even atoms, down for odd ones) for
    x-hat: every atom ends offset sqrt(3) from its place.  Records its calls."""

    device = torch.device("cpu")
    mean_center = True
    average_squared_distance = 0.332

    def __init__(self, offset_nm=0.0):
        self.calls, self.offset = [], offset_nm

    def noise_and_denoise(self, x, sigma, align_noisy_input, noise=None, rng="philox"):
        self.calls.append((x.dataset_label[0], float(sigma), x.num_graphs, bool(align_noisy_input), rng))
        from jamun_amd import native_denoise as nd

        sign = 1.0 - 2.0 * (torch.arange(x.num_nodes) % 2).float()
        return x.with_pos(nd.mean_center_graphs(x.pos, x.ptr) + self.offset * sign[:, None]), x


def test_evaluate_denoiser_files_and_loop_order(tmp_path):
    from jamun_amd import denoise_eval, synth
    from jamun_amd.model import Denoiser

    dsets = [dc.FramesDataset(synth.random_chain(17, seed=0), "zeta", 5), dc.FramesDataset(synth.ag_dipeptide(), "alpha", 12)]
    off = 0.01
    model = _StubModel(off)
    out = str(tmp_path / "denoise")
    res = denoise_eval.evaluate_denoiser(model, dsets, [0.04, 0.4], num_frames=7, batch_size=4, align_noisy_input=False, seed=3, rng="torch_cpu", output_dir=out)
    # datasets in label order, each sigma, then batches; a short last batch is its own batch
    assert model.calls == [("alpha", 0.04, 4, False, "torch_cpu"), ("alpha", 0.04, 3, False, "torch_cpu"), ("alpha", 0.4, 4, False, "torch_cpu"),
                           ("alpha", 0.4, 3, False, "torch_cpu"), ("zeta", 0.04, 4, False, "torch_cpu"), ("zeta", 0.04, 1, False, "torch_cpu"),
                           ("zeta", 0.4, 4, False, "torch_cpu"), ("zeta", 0.4, 1, False, "torch_cpu")]
    assert sorted(os.listdir(out)) == ["alpha.npz", "summary.json", "zeta.npz"]
    for label, F in (("alpha", 7), ("zeta", 5)):
        z = np.load(os.path.join(out, f"{label}.npz"))
        assert sorted(z.files) == ["coordinate_loss", "raw_coordinate_loss", "scaled_rmsd", "sigma"]
        assert z["sigma"].tolist() == [0.04, 0.4]
        for si, sigma in enumerate((0.04, 0.4)):
            # |xhat - x| = off sqrt 3 for every atom
            assert z["scaled_rmsd"].shape == (2, F) and z["scaled_rmsd"].dtype == np.float32
            assert np.allclose(z["scaled_rmsd"][si], off / sigma, rtol=1e-4)
            assert np.allclose(z["raw_coordinate_loss"][si], 3 * off * off, rtol=1e-4)
            assert np.allclose(z["coordinate_loss"][si], 3 * off * off * float(Denoiser.loss_weight(sigma, 0.332)), rtol=1e-4)
            key = f"{label}/scaled_rmsd_per_dataset/sigma={sigma}"
            assert res[key] == float(z["scaled_rmsd"][si].astype(np.float64).mean())
    summary = json.load(open(os.path.join(out, "summary.json")))
    assert summary["metrics"] == res and summary["num_frames"] == {"alpha": 7, "zeta": 5} and summary["sigma_list"] == [0.04, 0.4]
    assert summary["align_noisy_input"] is False and summary["seed"] == 3 and summary["batch_size"] == 4
    assert len(res) == 2 * 2 * 3
    with pytest.raises(ValueError, match="sigma_list is empty"):
        denoise_eval.evaluate_denoiser(model, dsets, [], output_dir=None)


def test_command_line_composes_the_sample_config_and_reaches_the_forward(tmp_path, monkeypatch):
    """``python -m jamun_amd.denoise_eval`` on a PDB and a synthetic checkpoint: the config composes, the model and the dataset load, the
    run directory is entered, and without a GPU the first forward says so (test_gpu_denoise.py runs it to the end)."""
    from jamun_amd import denoise_eval, pdb, synth

    mol = dict(synth.ag_dipeptide(), elements=["N", "C", "C", "C", "O", "N", "C", "C", "O", "O"], residue_ids=[1] * 5 + [2] * 5)
    pdb_path = str(tmp_path / "uncapped_AG.pdb")
    pdb.write_pdb(pdb_path, mol, mol["pos"][None])
    (tmp_path / "ckpt").mkdir()
    torch.save(synth.synthetic_checkpoint(output_gain=0.05), str(tmp_path / "ckpt" / "last.ckpt"))
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("JAMUN_ROOT_PATH", str(tmp_path))
    seen = {}

    def fake(model, datasets, sigma_list, **kw):
        seen.update(kw, sigma_list=list(sigma_list), labels=[d.label() for d in datasets], cwd=os.getcwd(), model=type(model).__name__)
        return {}

    monkeypatch.setattr(denoise_eval, "evaluate_denoiser", fake)
    args = ["--config-dir=" + os.path.join(ROOT, "configs"), "experiment=sample_custom", f"++init_pdbs=[{pdb_path}]", "++checkpoint_dir=ckpt"]
    run_dir = denoise_eval.main(args + ["++sigma_list=[0.04,0.1]", "++num_frames=3", "++align_noisy_input=false", "seed=11"])
    assert seen["sigma_list"] == [0.04, 0.1] and seen["num_frames"] == 3 and seen["align_noisy_input"] is False and seen["seed"] == 11
    assert seen["labels"] == ["uncapped_AG"] and seen["model"] == "Denoiser" and seen["batch_size"] == 256 and seen["rng"] == "philox"
    assert os.path.samefile(seen["cwd"], run_dir) and os.getcwd() == str(tmp_path)
    denoise_eval.main(args + ["sigma=0.07", "run_key=second"])  # sigma_list defaults to [${sigma}]
    assert seen["sigma_list"] == [0.07] and seen["num_frames"] is None and seen["align_noisy_input"] is True
