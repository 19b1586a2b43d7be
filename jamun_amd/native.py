"""Thin object wrappers over the C ABI (``include/jamun_hip.h``): model / sampler handles and the stand-alone operators (the entries of
``csrc/jamun_api.cpp``).  The calls that encode or analyse frames of a trajectory (``csrc/jamun_frames.cpp``) live in `native_frames`;
their public names are handed out here as well, so ``native.superpose_frames`` and the rest keep working; the two ends of a denoising
evaluation (``csrc/jamun_denoise.cpp``) live in `native_denoise` and are handed out here too.

PyTorch is used only for device memory and streams: every call passes ``tensor.data_ptr()`` and
``torch.cuda.current_stream().cuda_stream`` to the HIP library.
"""

from __future__ import annotations

import ctypes as C
import os
import functools
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .data import WalkerBatch
from .native_frames import (  # noqa: F401 (every public name it defines)
    pdb_models_nbytes, encode_pdb_models, encode_dcd_frames, superpose_frames, INTCOORD_FEATURE_TILE, check_index_table, internal_coords,
    HIST_SLICE, HIST_MAX_BINS, HIST_MAX_CUTS, hist_edges, check_cuts, check_hist_args, hist2d_pairs, js_divergence, VALIDITY_MAX_ATOMS,
    VALIDITY_CHUNK, VALIDITY_SPLIT_ATOMS, check_validity_tables, upload_validity_tables, validity_counts, TICA_MAX_WIDTH, TICA_MAX_ACF_LAG,
    TICA_SLICE, TICA_TILE, check_feature_rows, lagged_moments, project_frames, autocov_sums, MSM_MAX_K, MSM_MAX_D, MSM_MAX_KD, MSM_MAX_STATES,
    MSM_MAX_SEGMENTS, check_centers_shape, assign_centers, cluster_sums, transition_counts, label_counts, SWD_TILE, SWD_MAX_WIDTH, SWD_MAX_PROJ,
    check_swd_shapes, swd_project, swd_sort_segments, swd_merge, swd_w2sq,
)
from .native_denoise import noise_align_graphs, denoise_loss, noise_align_graphs_host, denoise_loss_host  # noqa: F401
from .native_frames import _ptr, _result, _state_map, _stream, _table, _work, _workspace  # noqa: F401 (all but _ptr, _stream: tests reach them here)


@functools.lru_cache(maxsize=None)
def normalize2mom_const(name: str) -> float:
    """e3nn ``normalize2mom`` constant: E_{z~N(0,1)}[f(z)^2]^(-1/2) from 1e6 float64 draws of ``Generator().manual_seed(0)``.

    These Python floats are not stored in checkpoints (e3nn recomputes them at module construction), so the
    loader recomputes them the same way.
    """
    f = {"leaky_relu": lambda z: torch.nn.functional.leaky_relu(z, 0.01), "sigmoid": torch.sigmoid}[name]
    gen = torch.Generator(device="cpu").manual_seed(0)
    z = torch.randn(1_000_000, generator=gen, dtype=torch.float64)
    cst = f(z).pow(2).mean().pow(-0.5).item()
    return 1.0 if abs(cst - 1) < 1e-4 else cst


def parse_hidden_irreps(s: str) -> Tuple[int, int]:
    m0 = m1 = 0
    for part in str(s).split("+"):
        part = part.strip()
        if not part:
            continue
        mul, ir = part.split("x") if "x" in part else ("1", part)
        ir = ir.strip()
        if ir == "0e":
            m0 += int(mul)
        elif ir == "1e":
            m1 += int(mul)
        else:
            raise NotImplementedError(f"irreps_hidden term {part!r}: only 0e and 1e irreps are supported")
    return m0, m1


def _dev_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); jamun_amd has no CPU path")
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(torch.float32).contiguous()
    return t


class NativeModel:
    """Owns a ``jamun_model*`` built from a reference-format state dict (names without the ``g.`` prefix)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], arch: dict, max_radius: float, average_squared_distance: float, mean_center: bool = True):
        lib = _lib.load()
        if str(arch.get("irreps_sh", "1x0e + 1x1e")).replace(" ", "") not in ("1x0e+1x1e",):
            raise NotImplementedError("only irreps_sh = 1x0e + 1x1e is supported")
        if str(arch.get("irreps_out", "1x1e")).replace(" ", "") not in ("1x1e", "1e"):
            raise NotImplementedError("only irreps_out = 1x1e is supported")
        if not arch.get("use_residue_information", True):
            raise NotImplementedError("SimpleAtomEmbedding (use_residue_information=False) is not supported")
        m0, m1 = parse_hidden_irreps(arch["irreps_hidden"])
        hp = _lib.jamun_hparams()
        hp.n_layers = int(arch["n_layers"])
        hp.mul0, hp.mul1 = m0, m1
        hp.edge_attr_dim = int(arch["edge_attr_dim"])
        dims = [arch["atom_type_embedding_dim"], arch["atom_code_embedding_dim"], arch["residue_code_embedding_dim"], arch["residue_index_embedding_dim"]]
        names = ["atom_type", "atom_code", "residue_code", "residue_index"]
        for i in range(4):
            hp.emb_dim[i] = int(dims[i])
            hp.emb_rows[i] = int(state_dict[f"atom_embedder.{names[i]}_embedding.weight"].shape[0])
        hp.use_residue_sequence_index = int(bool(arch.get("use_residue_sequence_index", False)))
        hp.mean_center = int(bool(mean_center))
        hp.max_radius = float(max_radius)
        hp.average_squared_distance = float(average_squared_distance)
        hp.act_scalar_const = normalize2mom_const("leaky_relu")
        hp.act_gate_const = normalize2mom_const("sigmoid")
        from .checkpoint import w3j_111_sign_from_state_dict

        hp.w3j_111_sign = w3j_111_sign_from_state_dict(state_dict)  # +1 unless the checkpoint's e3nn buffers say otherwise
        hp.separable = int(bool(arch.get("separable_conv", False)))
        self.hparams_struct = hp
        keep = []  # keep host buffers alive during the call
        arr = (_lib.jamun_tensor * len(state_dict))()
        n = 0
        for k, v in state_dict.items():
            if not torch.is_tensor(v) or not v.is_floating_point():
                continue
            t = v.detach().to("cpu", torch.float32).contiguous()
            keep.append(t)
            arr[n].name = k.encode()
            arr[n].data = C.cast(t.data_ptr(), C.POINTER(C.c_float))
            arr[n].numel = t.numel()
            n += 1
        handle = C.c_void_p()
        _lib.check(lib.jamun_model_create(C.byref(hp), arr, n, C.byref(handle)))
        self._h = handle
        self._lib = lib

    @property
    def handle(self):
        return self._h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.jamun_model_destroy(h)


# Kernel-selection switches (``jamun_tuning`` in include/jamun_hip.h) applied to every sampler created in this process.  Empty in
# production; tests set entries (``monkeypatch.setitem(native.TUNING, "no_mf", 1)``) to run one implementation of a block against another,
# and profiling scripts may set ``JAMUN_TUNING="no_mf,dg_kgroups=2"`` — the ONLY environment variable that reaches kernel selection,
# read here, once, at import (the C library reads none).
TUNING: dict = {}
for _item in filter(None, (os.environ.get("JAMUN_TUNING") or "").split(",")):
    _k, _, _v = _item.strip().partition("=")
    TUNING[_k] = int(_v) if _v else 1


def make_tuning(extra: Optional[dict] = None) -> "_lib.jamun_tuning":
    t = _lib.jamun_tuning()
    names = {n for n, _ in _lib.jamun_tuning._fields_} - {"reserved"}
    for k, v in {**TUNING, **(extra or {})}.items():
        if k not in names:
            raise ValueError(f"unknown tuning switch {k!r} (known: {sorted(names)})")
        setattr(t, k, int(v))
    return t


class NativeSampler:
    """Owns a ``jamun_sampler*``: packed weights for one sigma + work buffers for one walker batch."""

    def __init__(self, model: NativeModel, sigma: float, batch: WalkerBatch, device: torch.device, tuning: Optional[dict] = None):
        lib = _lib.load()
        if device.type != "cuda":
            raise RuntimeError("jamun_amd needs a GPU device (cuda / ROCm); there is no CPU path")
        self.device = device
        self.sigma = float(sigma)
        self.n_atoms = batch.num_nodes
        self.n_graphs = batch.num_graphs
        topo = _lib.jamun_topology()
        i32 = lambda t: t.detach().to("cpu", torch.int32).contiguous()
        keep = [i32(batch.ptr), i32(batch.atom_type_index), i32(batch.atom_code_index), i32(batch.residue_code_index), i32(batch.residue_sequence_index)]
        b = batch.bonds.detach().to("cpu", torch.int64).reshape(2, -1)
        bs, bd = b[0].contiguous(), b[1].contiguous()
        topo.n_atoms, topo.n_graphs = self.n_atoms, self.n_graphs
        pi = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_int32))
        topo.ptr, topo.atom_type_index, topo.atom_code_index, topo.residue_code_index, topo.residue_sequence_index = [pi(t) for t in keep]
        topo.n_bonds = int(bs.numel())
        topo.bond_src = C.cast(bs.data_ptr(), C.POINTER(C.c_int64))
        topo.bond_dst = C.cast(bd.data_ptr(), C.POINTER(C.c_int64))
        handle = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(lib.jamun_sampler_create(model.handle, C.c_float(self.sigma), C.byref(topo), C.byref(make_tuning(tuning)), C.byref(handle)))
        self._h = handle
        self._lib = lib
        self._model = model  # keep alive

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.jamun_sampler_destroy(h)

    def _new(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    def xhat(self, y: torch.Tensor) -> torch.Tensor:
        y = _dev_f32(y, "y")
        assert y.shape == (self.n_atoms, 3), y.shape
        out = self._new(self.n_atoms, 3)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.jamun_xhat(self._h, _ptr(y), _ptr(out), _stream()))
        return out

    def score(self, y: torch.Tensor) -> torch.Tensor:
        y = _dev_f32(y, "y")
        assert y.shape == (self.n_atoms, 3), y.shape
        out = self._new(self.n_atoms, 3)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.jamun_score(self._h, _ptr(y), _ptr(out), _stream()))
        return out

    def walk(self, integrator: str, y: torch.Tensor, v: torch.Tensor, params: "_lib.jamun_mcmc_params", noise: Optional[torch.Tensor], seed: int,
             save_trajectory: bool, want_xhat_traj: bool = True, want_xhat: bool = True):
        """Runs ``steps-1`` fused iterations on the current stream.  ``y`` and ``v`` are updated in place."""
        assert integrator in ("baoab", "aboba")
        ny, nsb, nsa = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self._lib.jamun_num_frames(C.byref(params), C.byref(ny), C.byref(nsb), C.byref(nsa)))
        n = self.n_atoms
        y_traj = score_traj = xhat_traj = None
        ns = nsb.value if integrator == "baoab" else nsa.value
        if save_trajectory:
            y_traj = self._new(ny.value, n, 3)
            xhat_traj = self._new(ny.value, n, 3) if want_xhat_traj else None
            score_traj = self._new(ns, n, 3)
        elif integrator == "baoab":
            score_traj = self._new(1, n, 3)  # the reference always keeps the initial score (_splitting.py:155)
        xhat = self._new(n, 3) if want_xhat else None
        if noise is not None:
            noise = _dev_f32(noise, "noise")
            assert noise.shape == (max(params.steps - 1, 0), n, 3), noise.shape
        fn = self._lib.jamun_walk_baoab if integrator == "baoab" else self._lib.jamun_walk_aboba
        with torch.cuda.device(self.device):
            _lib.check(fn(self._h, _ptr(y), _ptr(v), C.byref(params), _ptr(noise), C.c_uint64(seed & (2**64 - 1)),
                          _ptr(y_traj), _ptr(score_traj), _ptr(xhat_traj), _ptr(xhat), _stream()))
        return y_traj, score_traj, xhat_traj, xhat

    def check(self) -> None:
        """Synchronise and raise if a conv kernel flagged an edge table it cannot represent (``jamun_sampler_check``)."""
        with torch.cuda.device(self.device):
            _lib.check(self._lib.jamun_sampler_check(self._h, _stream()))

    def stats(self) -> dict:
        st = _lib.jamun_stats()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.jamun_sampler_stats(self._h, C.byref(st), _stream()))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def profile_enable(self, on: bool = True, classes=None, every: int = 1) -> None:
        """Record HIP events around the forward's launches: all classes, or only the named ones (``_lib.PROF_CLASSES``); ``every`` > 1
        samples every ``every``-th launch of a class instead of all of them (``jamun_profile_sample``)."""
        code = int(bool(on))
        if on and classes is not None:
            code = 0
            for c in classes:
                code |= 1 << (_lib.PROF_CLASSES.index(c) + 1)
        _lib.check(self._lib.jamun_profile_sample(self._h, int(every)))
        _lib.check(self._lib.jamun_profile_enable(self._h, code))

    def profile_read(self) -> dict:
        """{class: (total_ms, launches)} from HIP events recorded on the launch stream; synchronises the stream."""
        n = len(_lib.PROF_CLASSES)
        ms = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.jamun_profile_read(self._h, ms, cnt, _stream()))
        return {name: (ms[i], cnt[i]) for i, name in enumerate(_lib.PROF_CLASSES)}

    def build_edges(self, y: torch.Tensor) -> None:
        """``jamun_build_edges``: radius graph + bonded edges, edge geometry and the radial MLPs' hidden layer for positions
        ``y`` (``Denoiser.add_edges`` + ``E3Conv.forward`` up to the blocks); the edge table stays inside the sampler."""
        y = _dev_f32(y, "y")
        assert y.shape == (self.n_atoms, 3)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.jamun_build_edges(self._h, _ptr(y), _stream()))

    def conv_block(self, layer: int, x_in: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``jamun_conv_block``: one block of ``E3Conv`` on caller-owned node features and the current edge table — layer 0: the
        initial projector on the sampler's own noise-scaled embedding (``x_in`` must be None); layer l >= 1:
        ``w_l x + (1 - w_l) ConvBlock_l(s_l x)`` for ``x_in [n_atoms, mul0 + 3 mul1]``."""
        hp = self._model.hparams_struct
        out = self._new(self.n_atoms, hp.mul0 + 3 * hp.mul1)
        if x_in is not None:
            x_in = _dev_f32(x_in, "x_in")
            assert x_in.shape == out.shape, x_in.shape
        with torch.cuda.device(self.device):
            _lib.check(self._lib.jamun_conv_block(self._h, int(layer), _ptr(x_in), _ptr(out), _stream()))
        return out

    def debug_read(self, what: int, layer: int = 0) -> torch.Tensor:
        width = {0: None, 1: 1, 2: 3}[what]
        if what == 0:
            hp = self._model.hparams_struct
            width = hp.mul0 + 3 * hp.mul1
        out = self._new(self.n_atoms, width)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.jamun_debug_read(self._h, what, layer, _ptr(out), _stream()))
        return out

    def debug_segments(self, which: int) -> tuple:
        """``jamun_debug_segments``: a work list the destination-grouped kernels run, copied to the host — (int32 numpy array, info dict).
        which 0 / 1: segment records [grid, max_segs, 2, 4] of the hidden layers / the initial projector (empty: it runs list 0); 2: tail-tile
        records [n_tail_tiles, 4]; 3: tile table [n_tiles, 4]; 4 / 5: partial slabs per atom of list 0 / 1."""
        import numpy as np

        info = (C.c_int32 * 9)()
        _lib.check(self._lib.jamun_debug_segments(self._h, int(which), None, 0, info))
        n = int(info[0])
        out = np.zeros(max(n, 1), dtype=np.int32)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.jamun_debug_segments(self._h, int(which), out.ctypes.data_as(C.c_void_p), out.size, info))
        keys = ("n_values", "grid", "max_segs", "n_slabs", "ng", "n_k", "n_tiles", "seg_cost_tenths", "tail_runs")
        meta = {k: int(info[i]) for i, k in enumerate(keys)}
        out = out[:n]
        if which in (0, 1):
            out = out.reshape(meta["grid"], meta["max_segs"], 2, 4) if n else out.reshape(0, 0, 2, 4)
        elif which in (2, 3):
            out = out.reshape(-1, 4)
        return out, meta


def plan_segments(cus: int, ng: int, n_k: int, n_atoms: int, tile_atoms, tile_chunk, tile_weight, skip=None, seg_cost: float = 0.0) -> dict:
    """``jamun_debug_plan_segments``: the work-list planner of jamun_sampler_create, run on the host on the given tiles (no GPU needed).
    tile_atoms [n_tiles, 2] {first atom, atoms}; tile_chunk [n_tiles]; tile_weight [n_tiles] (>= 1); skip [n_tiles] or None.
    Returns {"segs": int32 [cus, max_segs, 2, 4], "max_segs", "n_slabs", "atom_nslab": int32 [n_atoms]}."""
    import numpy as np

    lib = _lib.load()
    ta = np.ascontiguousarray(tile_atoms, dtype=np.int32).reshape(-1, 2)
    n_tiles = ta.shape[0]
    tc = np.ascontiguousarray(tile_chunk, dtype=np.int32).reshape(n_tiles)
    tw = np.ascontiguousarray(tile_weight, dtype=np.int64).reshape(n_tiles)
    sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.int8).reshape(n_tiles)
    n_chunks = int(tc.max()) + 1 if n_tiles else 0
    ms, nsl = C.c_int32(), C.c_int32()
    nslab = np.zeros(max(n_atoms, 1), dtype=np.int32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    args = (int(cus), int(ng), int(n_k), int(n_atoms), n_tiles, vp(ta), vp(tc), n_chunks, vp(tw), vp(sk), float(seg_cost))
    segs = np.zeros((int(cus), 16, 2, 4), dtype=np.int32)
    code = lib.jamun_debug_plan_segments(*args, vp(segs), segs.size, C.byref(ms), C.byref(nsl), vp(nslab))
    if code != 0 and ms.value > segs.shape[1]:  # (longer lists than the first guess: max_segs is written, plan into a buffer of that size)
        segs = np.zeros((int(cus), ms.value, 2, 4), dtype=np.int32)
        code = lib.jamun_debug_plan_segments(*args, vp(segs), segs.size, C.byref(ms), C.byref(nsl), vp(nslab))
    _lib.check(code)
    segs = segs.reshape(-1)[: int(cus) * ms.value * 8].reshape(int(cus), ms.value, 2, 4).copy()
    return {"segs": segs, "max_segs": ms.value, "n_slabs": nsl.value, "atom_nslab": nslab[:n_atoms].copy()}


SELECT_KEYS = ("conv_path", "dg_mode", "init_path", "dg_emu", "dg_RS", "S", "n_tiles", "span_max", "row_blocks", "n_tail_tiles", "n_tail", "tail_runs",
               "init_tail", "own_init_segs", "mf_nks", "ml_window", "initv_nbuf", "ng", "seg_cost_tenths", "max_segs", "n_slabs",
               "conv_flop_exec_launch", "init_max_segs", "init_n_slabs")
SELECT_LISTS = ("segs", "init_segs", "tail_tiles", "tiles", "atom_nslab", "init_atom_nslab", "chunk")


def select_kernels(hp: dict, tuning: Optional[dict], ptr, bonds, cus: int, n_uniq: int, have_atom_uid: bool, hidden, layer0, lists=()) -> dict:
    """``jamun_debug_select_kernels``: the kernel selection of jamun_sampler_create, run on the host (no GPU needed).  hp: fields of
    ``jamun_hparams`` (the ones left out are zero; selection reads the widths, n_layers, edge_attr_dim, emb_dim and separable); tuning: switches
    as for ``NativeSampler`` (``TUNING`` is not applied); ptr [n_graphs + 1]; bonds [2, n_bonds]; hidden: per hidden layer (dg, mf, tail)
    flags; layer0: (tt2, tabw, tab_ut, wx, nt0).  Returns {name: int for SELECT_KEYS} plus the int32 arrays named in ``lists``
    (SELECT_LISTS; segs / init_segs [cus, max_segs, 2, 4], tail_tiles / tiles [n, 4])."""
    lib = _lib.load()
    h = _lib.jamun_hparams()
    for k, v in hp.items():
        if k == "emb_dim":
            for i in range(4):
                h.emb_dim[i] = int(v[i])
        else:
            setattr(h, k, v)
    t = _lib.jamun_tuning()
    for k, v in (tuning or {}).items():
        setattr(t, k, int(v))
    p = np.ascontiguousarray(ptr, dtype=np.int32)
    b = np.ascontiguousarray(bonds, dtype=np.int64).reshape(2, -1)
    bs, bd = np.ascontiguousarray(b[0]), np.ascontiguousarray(b[1])
    topo = _lib.jamun_topology()
    topo.n_atoms, topo.n_graphs, topo.n_bonds = int(p[-1]), p.size - 1, bs.size
    topo.ptr = p.ctypes.data_as(C.POINTER(C.c_int32))
    topo.bond_src, topo.bond_dst = bs.ctypes.data_as(C.POINTER(C.c_int64)), bd.ctypes.data_as(C.POINTER(C.c_int64))
    hid = np.ascontiguousarray([int(d) | int(m) << 1 | int(tl) << 2 for d, m, tl in hidden], dtype=np.int32)
    l0 = np.ascontiguousarray([int(x) for x in layer0], dtype=np.int32)
    out = np.zeros(len(SELECT_KEYS), dtype=np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    n = C.c_int64()

    def call(which, buf):
        _lib.check(lib.jamun_debug_select_kernels(C.byref(h), C.byref(t), C.byref(topo), int(cus), int(n_uniq), int(bool(have_atom_uid)), hid.size,
                                                  vp(hid), vp(l0), vp(out), which, None if buf is None else vp(buf), 0 if buf is None else buf.size, C.byref(n)))

    call(-1, None)
    res = {k: int(out[i]) for i, k in enumerate(SELECT_KEYS)}
    for name in lists:
        which = SELECT_LISTS.index(name)
        call(which, None)
        buf = np.zeros(max(n.value, 1), dtype=np.int32)
        call(which, buf)
        buf = buf[: n.value]
        if which in (0, 1):
            buf = buf.reshape(int(cus), -1, 2, 4) if buf.size else buf.reshape(0, 0, 2, 4)
        res[name] = buf.reshape(-1, 4) if which in (2, 3) else buf
    return res


def live_allocations() -> tuple:
    """``jamun_debug_live_allocations``: (number, bytes) of the device and pinned buffers the library holds in this process."""
    n, b = C.c_int64(), C.c_int64()
    _lib.check(_lib.load().jamun_debug_live_allocations(C.byref(n), C.byref(b)))
    return n.value, b.value


# ---- stand-alone operators --------------------------------------------------------------------------------------


def mean_center(pos: torch.Tensor, ptr: torch.Tensor) -> torch.Tensor:
    """``jamun.utils.mean_center`` on device (``src/jamun/utils/mean_center.py:7-12``)."""
    lib = _lib.load()
    pos = _dev_f32(pos, "pos")
    ptr = ptr.to(pos.device, torch.int32).contiguous()
    out = torch.empty_like(pos)
    with torch.cuda.device(pos.device):
        _lib.check(lib.jamun_mean_center(_ptr(pos), _ptr(ptr), ptr.numel() - 1, _ptr(out), _stream()))
    return out


def radius_graph(pos: torch.Tensor, r: float, ptr: torch.Tensor, stride: int = 33):
    """Neighbour table ``(nbr [N,stride] i32, deg [N] i32)``; see ``jamun_radius_graph``."""
    lib = _lib.load()
    pos = _dev_f32(pos, "pos")
    ptr = ptr.to(pos.device, torch.int32).contiguous()
    n = pos.shape[0]
    nbr = torch.full((n, stride), -1, dtype=torch.int32, device=pos.device)
    deg = torch.zeros(n, dtype=torch.int32, device=pos.device)
    with torch.cuda.device(pos.device):
        _lib.check(lib.jamun_radius_graph(_ptr(pos), _ptr(ptr), ptr.numel() - 1, n, C.c_float(r), stride, _ptr(nbr), _ptr(deg), _stream()))
    return nbr, deg


def radius_graph_edge_index(pos: torch.Tensor, r: float, ptr: torch.Tensor) -> torch.Tensor:
    """``edge_index [2,E]`` (src = neighbour, dst = centre), ordered by centre then neighbour — the reference layout."""
    nbr, deg = radius_graph(pos, r, ptr)
    n, s = nbr.shape
    mask = torch.arange(s, device=nbr.device)[None, :] < deg[:, None]
    dst = torch.arange(n, device=nbr.device)[:, None].expand(n, s)[mask]
    src = nbr[mask].long()
    return torch.stack([src, dst.long()])


def edge_geometry(pos_scaled: torch.Tensor, edge_index: torch.Tensor, radial_cutoff: float, n_basis: int = 32):
    """``(edge_sh [E,4], radial [E,n_basis])`` of ``E3Conv.forward`` (``arch/e3conv.py:114-123``) for an explicit edge list
    ``edge_index [2,E]`` (src, dst) and positions already scaled by ``c_in``; see ``jamun_edge_geometry``."""
    lib = _lib.load()
    pos = _dev_f32(pos_scaled, "pos_scaled")
    ei = edge_index.to(pos.device, torch.int64).contiguous()
    E = int(ei.shape[1])
    sh = torch.empty((E, 4), dtype=torch.float32, device=pos.device)
    radial = torch.empty((E, n_basis), dtype=torch.float32, device=pos.device)
    with torch.cuda.device(pos.device):
        _lib.check(lib.jamun_edge_geometry(_ptr(pos), int(pos.shape[0]), _ptr(ei[0].contiguous()), _ptr(ei[1].contiguous()), E,
                                           C.c_float(radial_cutoff), n_basis, _ptr(sh), _ptr(radial), _stream()))
    return sh, radial


def node_linear(x: torch.Tensor, weight: torch.Tensor, in0: int, in1: int, out0: int, out1: int) -> torch.Tensor:
    """e3nn ``o3.Linear`` between ``in0 x0e + in1 x1e`` and ``out0 x0e + out1 x1e`` with the flat e3nn weight; see ``jamun_node_linear``."""
    lib = _lib.load()
    x = _dev_f32(x, "x")
    w = _dev_f32(weight, "weight")
    assert x.shape[1] == in0 + 3 * in1, x.shape
    out = torch.empty((x.shape[0], out0 + 3 * out1), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.jamun_node_linear(_ptr(x), x.shape[0], in0, in1, out0, out1, _ptr(w), int(w.numel()), _ptr(out), _stream()))
    return out


def philox_normal(n: int, seed: int, iteration: int, device, first_atom: int = 0) -> torch.Tensor:
    """``[n, 3]`` standard-normal draws of integrator iteration ``iteration`` under ``seed``: exactly what the walks use in place of
    the reference's ``torch.randn_like`` (``functional/_splitting.py:161``) when no noise tensor is passed; see ``jamun_philox_normal``."""
    lib = _lib.load()
    device = torch.device(device)
    out = torch.empty((n, 3), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.jamun_philox_normal(_ptr(out), int(n), C.c_uint64(seed & (2**64 - 1)), C.c_uint32(iteration), C.c_uint32(first_atom), _stream()))
    return out


def scatter_mean(src: torch.Tensor, seg_ptr: torch.Tensor, n_out: int) -> torch.Tensor:
    """Mean of destination-sorted rows: ``out[d] = mean(src[seg_ptr[d]:seg_ptr[d+1]])`` (empty -> 0)."""
    lib = _lib.load()
    src = _dev_f32(src, "src")
    seg_ptr = seg_ptr.to(src.device, torch.int32).contiguous()
    assert seg_ptr.numel() == n_out + 1
    width = int(src.shape[1]) if src.ndim > 1 else 1
    out = torch.empty((n_out, width), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(lib.jamun_scatter_mean(_ptr(src), _ptr(seg_ptr), n_out, width, _ptr(out), _stream()))
    return out


def make_mcmc_params(steps, delta, friction, M, inverse_temperature, score_fn_clip, save_every_n_steps=1, burn_in_steps=0):
    p = _lib.jamun_mcmc_params()
    p.steps = int(steps)
    p.save_every_n_steps = int(save_every_n_steps)
    p.burn_in_steps = int(burn_in_steps)
    p.has_clip = int(score_fn_clip is not None)
    p.delta, p.friction, p.M = float(delta), float(friction), float(M)
    p.inverse_temperature = float(inverse_temperature)
    p.score_fn_clip = float(score_fn_clip) if score_fn_clip is not None else 0.0
    return p


def baoab_pre(y, v, psi, noise, params):
    lib = _lib.load()
    with torch.cuda.device(y.device):
        _lib.check(lib.jamun_baoab_pre(_ptr(y), _ptr(v), _ptr(psi), _ptr(noise), y.shape[0], C.byref(params), _stream()))


def baoab_post(v, psi, score, params):
    lib = _lib.load()
    with torch.cuda.device(v.device):
        _lib.check(lib.jamun_baoab_post(_ptr(v), _ptr(psi), _ptr(score), v.shape[0], C.byref(params), _stream()))


def aboba_a(y, v, params):
    lib = _lib.load()
    with torch.cuda.device(y.device):
        _lib.check(lib.jamun_aboba_a(_ptr(y), _ptr(v), y.shape[0], C.byref(params), _stream()))


def aboba_b(y, v, score, noise, params):
    lib = _lib.load()
    with torch.cuda.device(y.device):
        _lib.check(lib.jamun_aboba_b(_ptr(y), _ptr(v), _ptr(score), _ptr(noise), y.shape[0], C.byref(params), _stream()))
