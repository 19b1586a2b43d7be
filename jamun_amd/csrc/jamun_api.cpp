// jamun_api.cpp — host runtime behind include/jamun_hip.h: sampler create (allocation and upload of what jamun_pack.cpp packed and
// jamun_plan.cpp selected), work-buffer management, the per-step launch sequence, and the C ABI of the model, the sampler and the
// stand-alone operators.  The entries that analyse or encode frames and never touch a jamun_sampler are in jamun_frames.cpp.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "jamun_host.h"

namespace {

struct ProfScope {
  jamun_sampler* s; int cls; hipStream_t st; int b = -1;
  ProfScope(jamun_sampler* s_, int cls_, hipStream_t st_) : s(s_), cls(cls_), st(st_) {
    if (!(s->prof_mask >> cls & 1u)) return;
    if (s->prof_seen[cls]++ % s->prof_every != 0) return;
    while (s->ev_pool.size() < s->ev_next + 2) {
      hipEvent_t e;
      HIPCHECK(hipEventCreate(&e));
      s->ev_pool.push_back(e);
    }
    b = (int)s->ev_next;
    s->ev_next += 2;
    HIPCHECK(hipEventRecord(s->ev_pool[b], st));
  }
  ~ProfScope() {
    if (b < 0) return;
    (void)hipEventRecord(s->ev_pool[b + 1], st);
    s->ev_used.push_back({cls, {b, b + 1}});
  }
};

// Radial MLPs' hidden activations (k_edge_h; they depend on the geometry only) of n_layers blocks from block l0 on
void edge_h(jamun_sampler* s, size_t l0, int n_layers, hipStream_t st) {
  ProfScope ps(s, JAMUN_PROF_EDGE_H, st);
  if (s->plan.conv_path != CONV_WIDE) {
    launch_edge_h(s->deg, s->esrc, s->egeo, s->n_atoms, s->S, s->w1r_all + l0 * 64 * 32, s->cmask_all + l0 * 128, n_layers, s->mu, s->rb_step, s->h,
                  s->h_stride, s->h_kstride, st, s->w1h_all ? s->w1h_all + l0 * 8 * 64 : nullptr, s->w1isc_all ? s->w1isc_all + l0 : nullptr);
    return;
  }
  EdgeHWideArgs e{};
  e.deg = s->deg; e.esrc = s->esrc; e.egeo = s->egeo; e.n_atoms = s->n_atoms; e.S = s->S;
  e.H = s->hp.edge_attr_dim; e.nr = (s->hp.edge_attr_dim + 1) / 2; e.layer0 = (int)l0;
  e.w1r_all = s->w1r_all; e.cmask_all = s->cmask_all; e.mu = s->mu; e.step = s->rb_step;
  e.h_all = s->h + (s->h_batched ? l0 * s->h_stride : 0);  // (that block's table)
  e.h_layer_stride = s->h_stride; e.h_kstride = s->h_kstride;
  launch_edge_h_wide(e, n_layers, st);
}

// Geometry of one forward: centring, radius graph + bonded edges, unit vectors and distances (k_geom; `pre`: the first half of a
// BAOAB iteration fused in front of it), and — when the buffer holds all layers — the radial MLPs of every layer.
void build_edges(jamun_sampler* s, float* y, hipStream_t st, const LangevinPre& pre = LangevinPre(), bool geom_done = false) {
  if (!geom_done) {  // (geom_done: the previous walk iteration's last launch, k_finalize_geom, already advanced y and built the edge table)
    ProfScope ps(s, JAMUN_PROF_GEOM, st);
    launch_geom(y, s->ptr, s->n_graphs, s->c_in, s->r2, s->S, s->bond_in_ptr, s->bond_in_src, s->hp.mean_center, s->yc,
                s->deg, s->esrc, s->egeo, s->epair, pre, st);
  }
  if (s->h_batched) edge_h(s, 0, (int)s->layers.size(), st);
  s->edges_built = true;
}

// ---- argument structs of the conv kernels ----------------------------------------------------------
// What every conv argument struct starts with: the edge table, the layer's radial activations, the edge stride
template <typename A>
A edge_args(const jamun_sampler* s, const float* h_l) {
  A a{};
  a.deg = s->deg; a.esrc = s->esrc; a.egeo = s->egeo; a.h = h_l; a.h_kstride = s->h_kstride; a.S = s->S;
  return a;
}
// ... and what the kernels on the host-planned tiles (select_kernels) share on top of it
template <typename A>
A tile_args(const jamun_sampler* s, const LayerDev& L, const float* h_l) {
  A a = edge_args<A>(s, h_l);
  a.n_pad = s->n_pad; a.nt0 = L.p0.nt; a.tile_span = s->dev.tile_span; a.tile_atoms = s->dev.tile_atoms;
  a.partial0 = s->partial0; a.partial1 = s->partial1;
  return a;
}
// ... of those, the matrix-formed ones (jamun_conv_mf.hip, jamun_conv_ml.hip): k_geom's pair table, the coefficient scale, the error flag
template <typename A>
A mf_args(const jamun_sampler* s, const LayerDev& L, const float* h_l) {
  A a = tile_args<A>(s, L, h_l);
  int e3 = 0;
  std::frexp(1.5 * (double)L.dg.hmax2, &e3);  // 3 max|h~| < 2^e3
  a.sC = std::max(-40, std::min(40, 14 - e3));
  a.epair = s->epair; a.err = s->dev.mf_err;
  return a;
}
// The work lists and slab counts of a layer on the tile plan: the initial projector's own lists when it keeps the tail tiles (init_segs),
// else the hidden layers'
struct SegLists { const int4* segs; int max_segs; const int* atom_nslab; int n_slabs; };
SegLists seg_lists(const jamun_sampler* s, bool initial) {
  if (initial && s->plan.own_init_segs) return {s->dev.init_segs, s->plan.init_segs.max_segs, s->dev.init_atom_nslab, s->plan.init_segs.n_slabs};
  return {s->dev.segs, s->plan.segs.max_segs, s->dev.atom_nslab, s->plan.segs.n_slabs};
}
// Tail tiles (k_tail_form* + k_tail_contract): the fields the hidden layers and the initial projector share; each adds its operands
TailArgs tail_args(const jamun_sampler* s, const LayerDev& L, const float* h_l) {
  TailArgs t = mf_args<TailArgs>(s, L, h_l);
  t.n_k = s->hp.edge_attr_dim + 1; t.tail_tiles = s->dev.tail_tiles;
  t.n_tail_tiles = s->plan.n_tail_tiles(); t.n_tail = s->plan.n_tail(); t.n_runs = s->plan.tail_runs; t.tail_atom = s->dev.tail_atom; t.tail_scale = s->dev.tail_scale;
  t.P = s->dev.tail_P;
  return t;
}
// the initial projector's operands formed from the feature rows (k_conv_mfx, k_conv_mlx)
template <typename A>
A init_x_args(const jamun_sampler* s, const LayerDev& L, const float* h_l) {
  A f = mf_args<A>(s, L, h_l);
  const SegLists sl = seg_lists(s, true);
  f.segs = sl.segs; f.max_segs = sl.max_segs;
  f.xph = L.xph; f.xpl = L.xpl; f.wx = L.wx; f.sX = L.x_sX; f.cf0 = L.xcf0; f.cf1 = L.xcf1;
  return f;
}
// the hidden layers' operands of k_conv_mf / k_conv_ml
template <typename A>
A hidden_mf_args(const jamun_sampler* s, const LayerDev& L, const float* h_l, const float* x_in, int XSin) {
  A f = mf_args<A>(s, L, h_l);
  f.x = x_in; f.XS = XSin; f.n_atoms = s->n_atoms; f.segs = s->dev.segs; f.max_segs = s->plan.segs.max_segs;
  f.wm = L.dg.wm; f.Tt = s->dev.T; f.t_stride = s->dev.tstride; f.sB = L.dg.sB; f.sTw = L.dg.sTw;
  f.gx = L.dg.gx; f.cf0 = L.dg.cf0; f.cf1 = L.dg.cf1; f.x1 = s->x1;
  return f;
}

void check_launch(int rcode, const char* what) {
  if (rcode != 0) throw Err(JAMUN_ERR_INVALID, what);
}

// ---- the conv of one block, by kernel family -------------------------------------------------------
// k_conv / k_conv_wide: one launch for the scalar rows, one for the vector rows
void conv_general(jamun_sampler* s, size_t l, const float* h_l, const float* x_in, int XSin, hipStream_t st) {
  const bool wide = s->plan.conv_path == CONV_WIDE;
  LayerDev& L = s->layers[l];
  ConvArgs a = edge_args<ConvArgs>(s, h_l);
  a.x = x_in; a.n_atoms = s->n_atoms; a.n_pad = s->n_pad; a.n_tiles = s->n_pad / 32; a.S4 = (s->S + 3) & ~3; a.XS = XSin;
  a.n_slices = s->n_slices;
  for (int pi = 0; pi < 2; ++pi) {
    ConvProblemDev& P = pi == 0 ? L.p0 : L.p1;
    if (P.nt == 0) continue;
    a.wpack = P.wpack; a.chunks = P.chunks; a.slice_ptr = P.slice_ptr; a.ublk = P.ublk; a.lane_xoff = P.lane_xoff;
    a.partial = pi == 0 ? s->partial0 : s->partial1;
    ProfScope ps(s, l == 0 ? (pi == 0 ? JAMUN_PROF_CONV0_INIT : JAMUN_PROF_CONV1_INIT) : (pi == 0 ? JAMUN_PROF_CONV0 : JAMUN_PROF_CONV1), st);
    const int rcode = wide ? launch_conv_wide(a, P.planes, P.nt, st) : launch_conv(a, P.planes, P.nt, st);
    if (rcode == -2)
      throw Err(JAMUN_ERR_INVALID, wide ? "walker batch needs more than 160 KiB of LDS per wide conv workgroup (edge stride too large)"
                                        : "walker batch needs more than 160 KiB of LDS per conv workgroup (edge stride too large)");
    check_launch(rcode, wide ? "unsupported wide conv tile configuration" : "unsupported conv tile configuration");
  }
}

void conv_separable(jamun_sampler* s, size_t l, const float* h_l, const float* x_in, int XSin, hipStream_t st) {
  LayerDev& L = s->layers[l];
  SepArgs f = edge_args<SepArgs>(s, h_l);
  f.x = x_in; f.n_atoms = s->n_atoms; f.XS = XSin;
  f.n0 = L.sep.n0; f.n1 = L.sep.n1; f.w2b = L.sep.w2b; f.cfw = L.sep.cfw; f.bias = L.sep.bias; f.sH = L.sep.sH; f.D = s->sep_D;
  f.wl0 = L.sep.wl0; f.wl1 = L.sep.wl1;
  f.G0 = s->hp.mul0 + s->hp.mul1; f.G1 = s->hp.mul1; f.nt0 = L.p0.nt; f.nt1 = L.p1.nt;
  f.partial0 = s->partial0; f.partial1 = s->partial1;
  ProfScope ps(s, l == 0 ? JAMUN_PROF_CONV0_INIT : JAMUN_PROF_CONV0, st);
  check_launch(launch_sep_conv(f, s->cus, st), "separable conv launch failed (irreps not supported)");
}

// The initial projector on the tile plan (INIT_V, INIT_MFI, INIT_MFX, INIT_MLX)
void conv_init_tiles(jamun_sampler* s, const float* h_l, hipStream_t st) {
  LayerDev& L = s->layers[0];
  const char* failed = "initial-projector conv launch failed (configuration not supported)";
  const SegLists sl = seg_lists(s, true);
  {
    ProfScope ps(s, JAMUN_PROF_CONV0_INIT, st);
    switch (s->plan.init_path) {
      case INIT_MFI: {
        MfiArgs f = mf_args<MfiArgs>(s, L, h_l);
        f.segs = sl.segs; f.max_segs = sl.max_segs;
        f.atom_uid = s->atom_uid; f.tabw = L.tabw; f.sB = L.tab_sB; f.ut = L.tab_ut;
        check_launch(launch_conv_mfi(f, s->cus, st), failed);
        break;
      }
      case INIT_MFX: {
        const MfxArgs f = init_x_args<MfxArgs>(s, L, h_l);
        check_launch(launch_conv_mfx(f, s->cus, st), failed);
        break;
      }
      case INIT_MLX: {
        MlxArgs f = init_x_args<MlxArgs>(s, L, h_l);
        f.window = s->plan.ml_window; f.mfma_count = nullptr;
        check_launch(launch_conv_mlx(f, s->cus, st), failed);
        break;
      }
      default: {  // INIT_V
        InitVArgs f = tile_args<InitVArgs>(s, L, h_l);
        f.PMAX = (s->S + 3) & ~3; f.RS = s->plan.dg_RS; f.nbuf = s->plan.initv_nbuf;
        f.segs = sl.segs; f.max_segs = sl.max_segs;
        f.atom_uid = s->atom_uid; f.tt2 = L.tt2; f.tt2_kstride = (size_t)L.tt_U * 192;
        f.dbg = 0;
        check_launch(launch_conv_initv(f, s->cus, st), failed);
        break;
      }
    }
  }
  if (s->plan.init_tail) {  // (INIT_MFI / INIT_MFX only: the tail tiles through k_tail_form_init / k_tail_contract)
    TailArgs t = tail_args(s, L, h_l);
    t.xph = L.xph; t.xpl = L.xpl; t.wx = L.wx; t.sX = L.x_sX; t.cf0 = L.xcf0; t.cf1t = L.xcf1;
    ProfScope pt(s, JAMUN_PROF_CONV1_INIT, st);
    check_launch(launch_conv_tail_init(t, st), "tail-tile conv launch failed (configuration not supported)");
  }
}

// A hidden layer on the tile plan (CONV_DG): the T pre-pass, then k_conv_mf (+ tail tiles), k_conv_ml or k_conv_dg by dg_mode
void conv_hidden_tiles(jamun_sampler* s, size_t l, const float* h_l, const float* x_in, int XSin, hipStream_t st) {
  LayerDev& L = s->layers[l];
  const bool mf = matrix_formed(s->plan.dg_mode);
  {
    ProfScope pt(s, JAMUN_PROF_TPROD, st);
    if (mf) launch_tprod(x_in, XSin, s->n_atoms, s->hp.edge_attr_dim + 1, L.dg.wt, L.dg.wth, L.dg.gT, L.dg.cfT, s->dev.T, s->dev.tstride, st, s->tune.no_tprod_t != 0);
    else launch_tprod(x_in, XSin, s->n_atoms, s->hp.edge_attr_dim + 1, L.dg.wt, s->plan.dg_emu ? L.dg.wth : nullptr, L.dg.gT, L.dg.cfT, s->dev.T, 0, st);
  }
  if (s->plan.dg_mode == DG_MF) {
    MfArgs f = hidden_mf_args<MfArgs>(s, L, h_l, x_in, XSin);
    f.nks = s->plan.mf_nks;
    {
      ProfScope ps(s, JAMUN_PROF_CONV0, st);
      check_launch(launch_conv_mf(f, s->cus, st), "matrix-formed conv launch failed (configuration not supported)");
    }
    if (s->plan.n_tail_tiles()) {
      TailArgs t = tail_args(s, L, h_l);
      t.x = x_in; t.XS = XSin; t.gx = L.dg.gx; t.wm = L.dg.wm; t.wmt = L.dg.wmt; t.cf0 = L.dg.cf0; t.cf1t = L.dg.cf1t;
      ProfScope pt(s, JAMUN_PROF_CONV1, st);
      check_launch(launch_conv_tail(t, st), "tail-tile conv launch failed (configuration not supported)");
    }
  } else if (s->plan.dg_mode == DG_ML) {
    MlArgs f = hidden_mf_args<MlArgs>(s, L, h_l, x_in, XSin);
    f.window = s->plan.ml_window; f.mfma_count = s->dev.ml_count;
    ProfScope ps(s, JAMUN_PROF_CONV0, st);
    check_launch(launch_conv_ml(f, s->cus, st), "large-span matrix-formed conv launch failed (configuration not supported)");
    ++s->ml_launches;
  } else {
    DgArgs f = tile_args<DgArgs>(s, L, h_l);
    f.x = x_in; f.XS = XSin; f.RS = s->plan.dg_RS; f.PMAX = (s->S + 3) & ~3;  // multiple of the forming batch
    f.segs = s->dev.segs; f.max_segs = s->plan.segs.max_segs;
    f.row_blocks = s->plan.tiles.row_blocks ? 1 : 0; f.alt = s->plan.dg_mode;
    f.wx = L.dg.wx; f.wd = L.dg.wd; f.wv = L.dg.wv; f.T = s->dev.T; f.n_atoms = s->n_atoms;
    f.emu = s->plan.dg_emu; f.wh = L.dg.wxh; f.sB = L.dg.sB; f.hmax2 = L.dg.hmax2;
    f.gx = L.dg.gx; f.cf0 = L.dg.cf0; f.cf1 = L.dg.cf1;
    f.dbg = 0;
    f.dump = nullptr;
    ProfScope ps(s, JAMUN_PROF_CONV0, st);
    check_launch(launch_conv_dg(f, s->cus, st), "destination-grouped conv launch failed (configuration not supported)");
  }
}

// gate + self-interaction + skip Linear of one block, and the noise-conditional skip mix (the partial slabs summed on the way in)
void node_update(jamun_sampler* s, size_t l, bool on_tiles, const float* x_in, int XSin, float* x_out, hipStream_t st) {
  LayerDev& L = s->layers[l];
  ProfScope ps(s, JAMUN_PROF_NODE, st);
  auto common = [&](auto n) {  // (what NodeArgs and NodeWideArgs share)
    n.partial0 = s->partial0; n.partial1 = s->partial1; n.deg = s->deg; n.x_in = x_in; n.x_out = x_out; n.mix = L.mix;
    n.cL = s->hp.act_scalar_const; n.cS = s->hp.act_gate_const;
    n.n_atoms = s->n_atoms; n.n_pad = s->n_pad; n.n_slices = s->n_slices; n.nt0 = L.p0.nt; n.nt1 = L.p1.nt;
    n.mul0 = s->hp.mul0; n.mul1 = s->hp.mul1; n.in0 = L.in0; n.in1 = L.in1; n.XSin = XSin;
    return n;
  };
  if (s->plan.conv_path == CONV_WIDE) {
    NodeWideArgs n = common(NodeWideArgs{});
    n.z0 = s->z0; n.z1 = s->z1; n.wn0 = L.wn0; n.wn1 = L.wn1; n.K0p = L.K0w; n.K1p = L.K1w;
    n.no0 = (s->hp.mul0 + 31) / 32; n.no1 = (s->hp.mul1 + 31) / 32;
    launch_node_wide(n, st);
    return;
  }
  NodeArgs n = common(NodeArgs{});
  n.wcat0 = L.wcat0; n.wcat1 = L.wcat1; n.K0p = L.K0p; n.K1p = L.K1p;
  n.max_slabs = s->n_slices;
  if (on_tiles) {  // (slabs of the tile plan)
    const SegLists sl = seg_lists(s, l == 0);
    n.atom_nslab = sl.atom_nslab; n.max_slabs = sl.n_slabs;
  }
  if (s->plan.conv_path == CONV_SEP) { n.n_slices = 1; n.max_slabs = 1; }  // SeparableConv writes the summed messages as ONE slab
  n.wh0 = L.wh0; n.wh1 = L.wh1; n.K0h = L.K0h; n.K1h = L.K1h;
  n.kga0 = L.kga0; n.kga1 = L.kga1; n.kgx = L.kgx; n.cg0 = L.cg0; n.cg1 = L.cg1;
  if (!s->tune.node_fp32 && node_update_h_supported(n)) launch_node_update_h(n, s->cus, st);  // (node_fp32: the v_mfma_f32_32x32x2_f32 kernel, A/B aid)
  else launch_node_update(n, st);
}

// One block of the network on the current edge table: ConvBlock l (conv contraction + gate + self-interaction + skip Linear)
// and, for the hidden layers, the noise-conditional input scaling and skip mix around it (e3conv.py:129-133).
void run_layer(jamun_sampler* s, size_t l, const float* x_in, int XSin, float* x_out, hipStream_t st) {
  const float* h_l = s->h + (s->h_batched ? l * s->h_stride : 0);
  if (!s->h_batched) edge_h(s, l, 1, st);  // (batches above 4 GiB of activations: one layer's radial MLP at a time)
  bool on_tiles = false;  // the conv ran on the tile plan: its slabs are the plan's, not the n_slices K-slices
  if (l == 0) {
    switch (s->plan.init_path) {
      case INIT_V: case INIT_MFI: case INIT_MFX: case INIT_MLX: conv_init_tiles(s, h_l, st); on_tiles = true; break;
      case INIT_SEP: conv_separable(s, l, h_l, x_in, XSin, st); break;
      case INIT_GENERAL: case INIT_WIDE: conv_general(s, l, h_l, x_in, XSin, st); break;
    }
  } else {
    switch (s->plan.conv_path) {
      case CONV_DG: conv_hidden_tiles(s, l, h_l, x_in, XSin, st); on_tiles = true; break;
      case CONV_SEP: conv_separable(s, l, h_l, x_in, XSin, st); break;
      case CONV_GENERAL: case CONV_WIDE: conv_general(s, l, h_l, x_in, XSin, st); break;
    }
  }
  node_update(s, l, on_tiles, x_in, XSin, x_out, st);
}

// k_conv_mf / k_conv_mfi set a device flag when an ordered (source, destination) pair carries more edges than one coefficient
// entry can hold (the host plan excludes such topologies at create time; the kernels still report what they see).  Every entry
// point that ran a forward copies the flag into a pinned word behind its work (no synchronisation); every entry point first looks
// at that word, so a disagreement between plan and kernel surfaces as JAMUN_ERR_INVALID at the next call after the copy landed —
// at the latest in jamun_sampler_stats, which synchronises — instead of as silently wrong coordinates.
void mf_err_check(jamun_sampler* s) {
  if (s->dev.mf_err_host && *(volatile int*)s->dev.mf_err_host != 0)
    throw Err(JAMUN_ERR_INVALID, (*(volatile int*)s->dev.mf_err_host & 2)
                                     ? "k_conv_mf: an edge's source lies outside the rows the selected instantiation multiplies (host plan and kernel disagree) — results of this sampler are invalid"
                                     : "k_conv_mf: more than three edges of one (source, destination) pair — results of this sampler are invalid");
}
void mf_err_fetch(jamun_sampler* s, hipStream_t st) {
  if (s->dev.mf_err && s->dev.mf_err_host) HIPCHECK(hipMemcpyAsync(s->dev.mf_err_host, s->dev.mf_err, sizeof(int), hipMemcpyDeviceToHost, st));
}

// One denoiser forward.  `pre` / `post`: the two halves of a BAOAB iteration fused into the first and the last kernel of the
// forward (y is then advanced in place before the geometry is built).
void forward(jamun_sampler* s, float* y, float* xhat, float* score, hipStream_t st, const LangevinPre& pre = LangevinPre(),
             const LangevinPost& post = LangevinPost(), const LangevinPre* next_pre = nullptr, bool geom_done = false) {
  build_edges(s, y, st, pre, geom_done);
  const float* x_in = s->x_emb;
  int XSin = s->n_emb;
  for (size_t l = 0; l < s->layers.size(); ++l) {
    run_layer(s, l, x_in, XSin, s->x[l], st);
    x_in = s->x[l];
    XSin = s->XS;
  }
  HeadArgs hd{};
  hd.x = x_in; hd.w_gate = s->w_gate; hd.w_vec = s->w_vec; hd.w_out = s->w_out; hd.g = s->g;
  hd.cS = s->hp.act_gate_const; hd.n_atoms = s->n_atoms; hd.mul0 = s->hp.mul0; hd.mul1 = s->hp.mul1;
  {
    ProfScope ps(s, JAMUN_PROF_HEAD, st);
    if (s->plan.conv_path == CONV_WIDE) launch_head_wide(hd, st);
    else launch_head(hd, st);
    if (next_pre)  // walk: this iteration's finalize and the next iteration's geometry in one launch
      launch_finalize_geom(y, s->yc, s->g, s->ptr, s->n_graphs, s->c_skip, s->c_out, s->sigma * s->sigma, s->hp.mean_center, s->tmp, xhat, score, post,
                           s->c_in, s->r2, s->S, s->bond_in_ptr, s->bond_in_src, s->deg, s->esrc, s->egeo, s->epair, *next_pre, st);
    else
      launch_finalize(y, s->yc, s->g, s->ptr, s->n_graphs, s->c_skip, s->c_out, s->sigma * s->sigma, s->hp.mean_center,
                      s->tmp, xhat, score, post, st);
  }
  HIPCHECK(hipGetLastError());
}

LangevinConsts make_consts(const jamun_mcmc_params* p) {
  if (p->M <= 0) throw Err(JAMUN_ERR_INVALID, "M must be positive");
  const double u = 1.0 / (double)p->M;  // pow(M, -1)
  const double zeta2 = std::sqrt(1.0 - std::exp(-2.0 * (double)p->friction));
  LangevinConsts k;
  k.u_half_delta = (float)(u * ((double)p->delta / 2));
  k.half_delta = (float)((double)p->delta / 2);
  k.exp_mg = (float)std::exp(-(double)p->friction);
  k.zeta_sqrt_u = (float)(zeta2 * std::sqrt(u));
  k.beta = p->inverse_temperature;
  k.clip = p->score_fn_clip;
  k.has_clip = p->has_clip;
  return k;
}

void check_mcmc(const jamun_mcmc_params* p) {
  if (!p) throw Err(JAMUN_ERR_INVALID, "null mcmc params");
  if (p->steps < 1) throw Err(JAMUN_ERR_INVALID, "steps must be >= 1");
  if (p->save_every_n_steps < 1) throw Err(JAMUN_ERR_INVALID, "save_every_n_steps must be >= 1");
}

bool saves(const jamun_mcmc_params* p, int i) { return (i % p->save_every_n_steps) == 0 && i >= p->burn_in_steps; }

// ---- FLOP and byte model: what create fixes per sampler (count_flops) and what needs the edge count of the batch (fill_stats_model) ----
void count_flops(jamun_sampler* s) {
  const jamun_hparams& hp = s->hp;
  const ConvModel cm = conv_model(s->plan, hp, s->n_atoms);
  for (auto& L : s->layers) {
    s->flop_ref_per_edge += 2LL * hp.edge_attr_dim * hp.edge_attr_dim + 2LL * (hp.edge_attr_dim + 1) * L.tp_numel;  // SURVEY.md §8 d (SeparableConv: tp_numel = the 336 depth-wise weights)
    if (s->plan.conv_path == CONV_DG && &L != &s->layers[0]) s->flop_exec += cm.conv_flop + cm.tprod_flop;
    else if (L.sep.w2b) s->flop_exec += 3LL * 2 * (int64_t)s->n_atoms * 32 * ((s->S + 31) / 32) * 64 * 352;  // the per-edge weight GEMM as f16x3 (the rest is VALU work per edge)
    else s->flop_exec += 2LL * s->n_pad * (1LL * L.p0.K * L.p0.nt * 32 + 3LL * L.p1.K * L.p1.nt * 32);
  }
}

// k_conv_ml counts its own MFMAs (block-sparse forming); the count stands for the model's figure once it has launched
bool ml_counted(const jamun_sampler* s) { return s->plan.conv_path == CONV_DG && s->plan.dg_mode == DG_ML && s->dev.ml_count && s->ml_launches > 0; }

// e: edges of the current table; ml_cnt: k_conv_ml's own count of its MFMAs (ml_counted; else unused)
void fill_stats_model(const jamun_sampler* s, int64_t e, unsigned long long ml_cnt, jamun_stats* out) {
  const int64_t m0 = s->hp.mul0, m1 = s->hp.mul1, H1 = s->hp.edge_attr_dim + 1, N = s->n_atoms;
  const bool dg = s->plan.conv_path == CONV_DG, mf = dg && matrix_formed(s->plan.dg_mode);
  const ConvModel cm = conv_model(s->plan, s->hp, s->n_atoms);
  out->flop_ref_assoc = e * s->flop_ref_per_edge;
  out->flop_executed = s->flop_exec;
  out->conv0_flop_alg = 2 * N * H1 * (m0 + m1) * (m0 + m1);
  out->conv1_flop_alg = 2 * 3 * N * H1 * (m0 + 2 * m1) * m1;
  out->conv_flop_exec_launch = (s->x1 && s->plan.dg_mode == DG_MF) ? cm.conv_flop / 3 : cm.conv_flop;
  if (ml_counted(s))  // (block-sparse forming: counted by the kernel; mean over its launches so far)
    out->conv_flop_exec_launch = (int64_t)((double)ml_cnt / (double)s->ml_launches) * 32768;
  if (dg && s->layers.size() > 1)  // one basis for both figures: the hidden layers' share of flop_executed follows the per-launch figure reported above (f16x1: a third; k_conv_ml: kernel-counted)
    out->flop_executed += (int64_t)(s->layers.size() - 1) * (out->conv_flop_exec_launch - cm.conv_flop);
  out->conv_flop_useful_launch = out->conv_bytes_alg_launch = 0;
  if (dg && s->layers.size() > 1) {
    // (the launch these figures describe is the main conv kernel: destinations that go through the tail kernels are not its work — their
    // edges are taken as the batch's mean in-degree, the slab and h~ bytes below stay whole: every slot is read, every slab row written)
    const int64_t Nm = N - s->plan.n_tail(), em = N > 0 ? (int64_t)((double)e * (double)Nm / (double)N) : 0;
    const int64_t contraction = 2 * H1 * Nm * ((m0 + m1) * (m0 + m1) + 3 * m1 * (2 * m1));
    // per edge and k: x0 (m0), dot 3 m1, x1 3 m1, cross 6 m1, T term 3 m1 — on the matrix cores only in k_conv_mf (k_conv_dg forms on the vector ALUs)
    const int64_t forming = mf ? 2 * H1 * em * (m0 + 15 * m1) : 0;
    out->conv_flop_useful_launch = (s->x1 ? 1 : s->plan.dg_emu ? 3 : 1) * (contraction + forming);
    const int64_t slots = (int64_t)s->h_kstride;
    out->conv_bytes_alg_launch = 4 * (H1 * slots          // h~ of the layer
                                      + H1 * 32 * N         // T
                                      + N * s->XS           // feature rows
                                      + (int64_t)s->plan.segs.n_slabs * s->n_pad * 32 * (s->layers[1].p0.nt + 3 * s->layers[1].p1.nt)) +  // slabs
                                 cm.weight_bytes;
  } else if (s->layers.size() > 1 && s->layers[1].sep.w2b) {
    // SeparableConv hidden layer (k_sep_fused + k_sep_linear): h~ of the layer, one feature row per edge, the per-destination sums written
    // and read once, the slab, W2~ and the Linear's weights once
    const int64_t n0 = s->layers[1].sep.n0, n1 = s->layers[1].sep.n1, DW = n0 + n1 + 3 * (n0 + 2 * n1);
    out->conv_bytes_alg_launch = 4 * (H1 * (int64_t)s->h_kstride + e * s->XS + 2 * N * DW + N * (160 + 96) +
                                      (n0 + n1) * (m0 + m1) + (n0 + 2 * n1) * m1) + 4 * 11 * 2 * 1024;
  }
}

// ---- sampler create, step by step (sampler_create_impl) ---------------------------------------------------------------------------
void set_max_lds() {
  const std::pair<const char*, int (*)()> lds_attr[] = {{"k_conv", conv_set_max_lds}, {"k_node_update", node_update_set_max_lds},
                                                        {"k_conv_init_v", conv_initv_set_max_lds}, {"k_conv_dg", conv_dg_set_max_lds},
                                                        {"k_tprod_t", tprod_set_max_lds}, {"jamun_conv_tail.hip", conv_tail_set_max_lds},
                                                        {"jamun_conv_mf.hip", conv_mf_set_max_lds}, {"jamun_conv_ml.hip", conv_ml_set_max_lds},
                                                        {"jamun_sepconv.hip", sep_conv_set_max_lds}, {"jamun_wide.hip", conv_wide_set_max_lds}};
  for (auto& f : lds_attr)
    if (f.second() != 0)
      throw Err(JAMUN_ERR_HIP, std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed for ") + f.first + ": " + hipGetErrorString(hipGetLastError()));
}

// radial basis centres: torch.linspace(0, r_cut, 34)[1:-1] in fp32 (e3nn soft_one_hot_linspace)
void upload_radial_centres(jamun_sampler* s) {
  const int nr = (s->hp.edge_attr_dim + 1) / 2, steps = nr + 2;
  const float start = 0.f, end = s->r_cut;
  const float step = (end - start) / (float)(steps - 1);
  std::vector<float> vals(steps);
  for (int i = 0; i < steps; ++i) vals[i] = (i < steps / 2) ? start + step * (float)i : end - step * (float)(steps - i - 1);
  s->rb_step = vals[1] - vals[0];
  std::vector<float> mu(vals.begin() + 1, vals.end() - 1);
  s->mu = s->mem.upload(mu);
}

struct Embeddings { std::vector<float> xe_host, uniq; std::vector<int> uid; };  // the scaled embedding row of every atom; the distinct ones; [n_atoms] index into them

// scaled atom embeddings (constant per topology and sigma): atom_embedding.py:58-76, noise_conditioning.py:50-54
Embeddings upload_embeddings(jamun_sampler* s, const jamun_model* m, const jamun_topology* topo, double c_noise) {
  const jamun_hparams& hp = s->hp;
  const int N = s->n_atoms;
  const char* names[4] = {"atom_embedder.atom_type_embedding.weight", "atom_embedder.atom_code_embedding.weight",
                          "atom_embedder.residue_code_embedding.weight", "atom_embedder.residue_index_embedding.weight"};
  const int32_t* idx[4] = {topo->atom_type_index, topo->atom_code_index, topo->residue_code_index, topo->residue_sequence_index};
  std::vector<double> s0 = noise_mlp(*m, "initial_noise_scaling.scale_predictor", s->n_emb, c_noise);
  Embeddings E;
  std::vector<float>& xe = E.xe_host;
  xe.assign((size_t)N * s->n_emb, 0.f);
  int col = 0;
  for (int tb = 0; tb < 4; ++tb) {
    const auto& T = m->get(names[tb], (int64_t)hp.emb_rows[tb] * hp.emb_dim[tb]);
    for (int i = 0; i < N; ++i) {
      int row = idx[tb][i];
      if (tb == 3 && !hp.use_residue_sequence_index) row = 0;
      if (row < 0 || row >= hp.emb_rows[tb]) throw Err(JAMUN_ERR_INVALID, std::string("index out of range for ") + names[tb]);
      for (int c = 0; c < hp.emb_dim[tb]; ++c)
        xe[(size_t)i * s->n_emb + col + c] = (float)((double)T[(size_t)row * hp.emb_dim[tb] + c] * s0[col + c]);
    }
    col += hp.emb_dim[tb];
  }
  s->x_emb = s->mem.upload(xe);
  // distinct rows of the scaled embedding (atoms with equal embedding indices share one): the initial projector's
  // input-times-weight products are tabulated per distinct row
  E.uid.resize(N);
  std::map<std::vector<float>, int> seen;
  for (int i = 0; i < N; ++i) {
    std::vector<float> row(xe.begin() + (size_t)i * s->n_emb, xe.begin() + (size_t)(i + 1) * s->n_emb);
    auto it = seen.find(row);
    if (it == seen.end()) {
      it = seen.emplace(row, (int)seen.size()).first;
      E.uniq.insert(E.uniq.end(), row.begin(), row.end());
    }
    E.uid[i] = it->second;
  }
  return E;
}

void build_layers(jamun_sampler* s, const jamun_model* m, const Embeddings& E, double c_noise, bool wide) {
  const jamun_hparams& hp = s->hp;
  {
    // initial projector: four scalar blocks (irreps not simplified, atom_embedding.py:54-56); scaling already in x_emb
    std::vector<InBlock> ib;
    int xo = 0;
    const int muls[4] = {hp.emb_dim[0], hp.emb_dim[0], hp.emb_dim[2], hp.emb_dim[3]};
    for (int b = 0; b < 4; ++b) { ib.push_back({muls[b], 0, xo, xo}); xo += muls[b]; }
    std::vector<double> ones(s->n_emb, 1.0);
    if (wide) s->layers.push_back(build_layer(s->mem, s->dg_mem, *m, "initial_projector", ib, ones, s->n_slices, nullptr, 0, false, nullptr, true));
    else s->layers.push_back(build_layer(s->mem, s->dg_mem, *m, "initial_projector", ib, ones, s->n_slices, &E.uniq, s->n_emb, false, &E.xe_host));
    s->n_uniq = (int)(E.uniq.size() / (size_t)std::max(s->n_emb, 1));
    if (s->layers.back().tt2 || s->layers.back().tabw) s->atom_uid = s->mem.upload(E.uid);
  }
  for (int l = 0; l < hp.n_layers; ++l) {
    std::vector<InBlock> ib = {{hp.mul0, 0, 0, 0}, {hp.mul1, 1, hp.mul0, hp.mul0}};
    const std::string li = std::to_string(l);
    std::vector<double> sc = noise_mlp(*m, "noise_scalings." + li + ".scale_predictor", hp.mul0 + hp.mul1, c_noise);
    LayerDev L = build_layer(s->mem, s->dg_mem, *m, "layers." + li, ib, sc, s->n_slices, nullptr, 0, /*pack_dg=*/!s->tune.no_dg && !wide, nullptr, wide);
    std::vector<double> wm = noise_mlp(*m, "skip_connections." + li + ".weights.scale_predictor", hp.mul0 + hp.mul1, c_noise);
    std::vector<float> mix(wm.size());
    for (size_t i = 0; i < wm.size(); ++i) mix[i] = (float)(1.0 / (1.0 + std::exp(-wm[i])));
    L.mix = s->mem.upload(mix);
    s->layers.push_back(L);
  }
  for (auto& L : s->layers)
    if (L.sep.w2b)
      if (const char* why = sep_conv_unsupported(L.sep.n0, L.sep.n1, L.p0.nt, L.p1.nt, s->S, hp.edge_attr_dim)) throw Err(JAMUN_ERR_INVALID, why);
}

// What packing did, as kernel selection asks it (the one place that looks at the layers' pointers for it)
PackedLayouts packed_layouts(const std::vector<LayerDev>& layers) {
  PackedLayouts p;
  for (size_t l = 1; l < layers.size(); ++l) p.hidden.push_back({layers[l].dg.wx != nullptr, layers[l].dg.wm != nullptr, layers[l].dg.wmt != nullptr});
  const LayerDev& L0 = layers[0];
  p.tt2 = L0.tt2 != nullptr; p.tabw = L0.tabw != nullptr; p.wx = L0.wx != nullptr; p.tab_ut = L0.tab_ut; p.nt0 = L0.p0.nt;
  return p;
}

// The sampler's plan onto the device: for CONV_DG the tile tables, tail tiles and work lists, and the buffers the plan sizes
void upload_plan(jamun_sampler* s) {
  DevArena& mem = s->mem;
  const KernelPlan& P = s->plan;
  PlanDev& d = s->dev;
  if (P.conv_path != CONV_DG) {  // the tile plan's weights are not needed: released now, not at destroy
    s->dg_mem.clear();
    for (auto& L : s->layers) L.dg = DgDev{};
    return;
  }
  const int N = s->n_atoms, n_k = s->hp.edge_attr_dim + 1;
  const TilePlan& T = P.tiles;
  if (P.n_tail_tiles()) {
    d.tail_tiles = mem.upload(P.tail_tiles);
    d.tail_atom = mem.upload(P.tail_atom);
    d.tail_scale = mem.alloc<float>(P.tail_atom.size());
    d.tail_P = mem.alloc<float4>(P.tail_P_bytes / 16);
  }
  // every segment record carries its tile's descriptor — {k_extra, first destination, destinations | source rows << 8, first source row} —
  // so that a kernel's first prologue is ONE round trip behind the segment list instead of two (list -> tile tables -> loads)
  auto upload = [&](const SegPlan& L, int4*& segs_dev, int*& atom_nslab) {
    std::vector<int4> segs = L.segs;
    for (size_t i = 0; i + 1 < segs.size(); i += 2) {
      const int t = segs[i].x;
      if (t < 0) continue;
      segs[i + 1].y = T.atoms[t].x;
      segs[i + 1].z = T.atoms[t].y | ((T.span[t].y - T.span[t].x) << 8);
      segs[i + 1].w = T.span[t].x;
    }
    segs_dev = mem.upload(segs); atom_nslab = mem.upload(L.atom_nslab);
  };
  if (P.own_init_segs) upload(P.init_segs, d.init_segs, d.init_atom_nslab);
  upload(P.segs, d.segs, d.atom_nslab);
  d.tile_atoms = mem.upload(T.atoms);
  d.tile_span = mem.upload(T.span);
  if (P.dg_mode == DG_ML) d.ml_count = mem.zeroed<unsigned long long>(1);
  if (matrix_formed(P.dg_mode)) {
    d.tstride = ((N + 31) & ~31) + 64;
    d.T = mem.zeroed<float>((size_t)n_k * 32 * d.tstride);
    d.mf_err = mem.zeroed<int>(1);
    d.mf_err_host = mem.pinned<int>(1);
    *d.mf_err_host = 0;
  } else {
    d.T = mem.alloc<float>((size_t)n_k * N * 32);
  }
  s->x1 = (s->tune.f16x1 && matrix_formed(P.dg_mode) && P.dg_emu) ? 1 : 0;
}

void alloc_work_buffers(jamun_sampler* s) {
  DevArena& mem = s->mem;
  const jamun_hparams& hp = s->hp;
  const bool wide = s->plan.conv_path == CONV_WIDE;
  const size_t N = (size_t)s->n_atoms, NS = N * s->S;
  for (float** p : {&s->yc, &s->g, &s->tmp, &s->xhat_buf, &s->score_buf, &s->psi}) *p = mem.alloc<float>(N * 3);
  s->deg = mem.alloc<int>(N);
  s->esrc = mem.alloc<int>(NS);
  s->epair = mem.zeroed<int>(NS);  // (pair table of the matrix-formed kernels, written by k_geom with the edges)
  s->egeo = mem.alloc<float4>(NS);
  std::vector<float> w1r_all, cmask_all;
  for (auto& L : s->layers) {
    w1r_all.insert(w1r_all.end(), L.w1r_h.begin(), L.w1r_h.end());
    cmask_all.insert(cmask_all.end(), L.cmask_h.begin(), L.cmask_h.end());
  }
  s->w1r_all = mem.upload(w1r_all);
  if (hp.edge_attr_dim == 64 && !s->tune.edge_h_fp32 && !wide) pack_edge_h16(s);
  s->cmask_all = mem.upload(cmask_all);
  s->h_kstride = (NS + 63) & ~(size_t)63;
  s->h_stride = s->h_kstride * (wide ? (size_t)hp.edge_attr_dim + 1 : (size_t)JAMUN_HROWS);  // (H + 1 rows)
  s->h_batched = s->h_stride * s->layers.size() * sizeof(float) <= ((size_t)4 << 30);  // all layers' h~ at once, up to 4 GiB
  // (+ slack: k_conv_mf reads h~ at slot0 + p * stride without a bounds test; lanes past the last atom's slots read up to
  // 32 * S + 128 floats beyond the table and never use them)
  s->h = mem.alloc<float>(s->h_stride * (s->h_batched ? s->layers.size() : 1) + 32 * (size_t)s->S + 256);
  int nt0 = 0, nt1 = 0;
  for (auto& L : s->layers) { nt0 = std::max(nt0, L.p0.nt); nt1 = std::max(nt1, L.p1.nt); }
  const size_t n_part = (size_t)std::max(std::max(s->n_slices, s->plan.segs.n_slabs), s->plan.init_segs.n_slabs);  // (1 each without a tile plan)
  s->partial0 = mem.alloc<float>(n_part * s->n_pad * nt0 * 32);
  s->partial1 = mem.alloc<float>(n_part * s->n_pad * 3 * nt1 * 32);
  {
    int dw = 0;
    for (auto& L : s->layers)
      if (L.sep.w2b) dw = std::max(dw, L.sep.n0 + L.sep.n1 + 3 * (L.sep.n0 + 2 * L.sep.n1));
    if (dw > 0) s->sep_D = mem.alloc<float>(N * dw);
  }
  if (wide) {
    int k0 = 8, k1 = 8;
    for (auto& L : s->layers) { k0 = std::max(k0, L.K0w); k1 = std::max(k1, L.K1w); }
    s->z0 = mem.zeroed<float>((size_t)s->n_pad * k0);
    s->z1 = mem.zeroed<float>((size_t)3 * s->n_pad * k1);
  }
  for (size_t l = 0; l < s->layers.size(); ++l) s->x.push_back(mem.alloc<float>(N * s->XS));
  s->counter = mem.alloc<unsigned long long>(1);
}

jamun_tuning checked_tuning(const jamun_tuning* tuning) {
  jamun_tuning tn{};
  if (tuning) tn = *tuning;
  if (tn.dg_kgroups != 0 && tn.dg_kgroups != 1 && tn.dg_kgroups != 2 && tn.dg_kgroups != 4 && tn.dg_kgroups != 8)
    throw Err(JAMUN_ERR_INVALID, "jamun_tuning.dg_kgroups must be 0 (default), 1, 2, 4 or 8");
  if (tn.f16x1 != 0 && tn.f16x1 != 1) throw Err(JAMUN_ERR_INVALID, "jamun_tuning.f16x1 must be 0 or 1");
  if (tn.seg_cost_tenths < -1 || tn.seg_cost_tenths > 1000) throw Err(JAMUN_ERR_INVALID, "jamun_tuning.seg_cost_tenths must be -1 (no segment cost), 0 (default) or 1..1000");
  return tn;
}

std::unique_ptr<jamun_sampler> sampler_create_impl(const jamun_model* m, float sigma, const jamun_topology* topo, const jamun_tuning* tuning) {
  const jamun_tuning tn = checked_tuning(tuning);
  if (!(sigma > 0)) throw Err(JAMUN_ERR_INVALID, "sigma must be positive");
  if (topo->n_atoms < 1 || topo->n_graphs < 1) throw Err(JAMUN_ERR_INVALID, "empty walker batch");
  const jamun_hparams& hp = m->hp;
  std::unique_ptr<jamun_sampler> s(new jamun_sampler());
  s->hp = hp; s->tune = tn; s->sigma = sigma;
  s->n_atoms = topo->n_atoms; s->n_graphs = topo->n_graphs;
  s->n_pad = ((topo->n_atoms + 31) / 32) * 32;
  s->XS = hp.mul0 + 3 * hp.mul1;
  s->n_emb = hp.emb_dim[0] + hp.emb_dim[1] + hp.emb_dim[2] + hp.emb_dim[3];
  const ConvPath base = base_conv_path(hp, s->n_emb);
  // ---- normalisation factors in fp32, op for op as Denoiser.normalization_factors (denoiser.py:116-136,177-178)
  {
    const float A = hp.average_squared_distance;
    const float B = 6.0f * (sigma * sigma);
    s->c_in = 1.0f / sqrtf(A + B);
    s->c_skip = A / (A + B);
    s->c_out = sqrtf((A * B) / (A + B));
    const float mr2 = (float)((double)hp.max_radius * (double)hp.max_radius);
    s->r_cut = sqrtf(mr2 + 6.0f * (sigma * sigma)) / s->c_in;
    s->r2 = s->r_cut * s->r_cut;
  }
  const double c_noise = std::log((double)sigma) / 4.0;
  const TopoHost th = check_topology(*topo);
  s->S = th.S;
  set_max_lds();
  s->ptr = s->mem.upload(std::vector<int>(topo->ptr, topo->ptr + topo->n_graphs + 1));
  s->bond_in_ptr = s->mem.upload(th.bip);
  s->bond_in_src = s->mem.upload(th.bis);
  upload_radial_centres(s.get());
  const Embeddings E = upload_embeddings(s.get(), m, topo, c_noise);
  build_layers(s.get(), m, E, c_noise, base == CONV_WIDE);
  pack_head(*m, s.get());
  int dev = 0, cus = 0;
  HIPCHECK(hipGetDevice(&dev));
  HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  s->cus = std::max(cus, 1);
  // ---- kernel selection (jamun_plan.cpp); upload of the tile plan and work lists of the destination-grouped kernels
  s->plan = select_kernels(hp, tn, *topo, th, s->cus, base, packed_layouts(s->layers), s->n_uniq, s->atom_uid != nullptr);
  upload_plan(s.get());
  alloc_work_buffers(s.get());
  count_flops(s.get());
  HIPCHECK(hipDeviceSynchronize());
  return s;
}

}  // namespace

extern "C" {

const char* jamun_last_error(void) { return jamun_error_slot.c_str(); }
int jamun_version(void) { return 6; }

int jamun_model_create(const jamun_hparams* hp, const jamun_tensor* tensors, int32_t n_tensors, jamun_model** out) {
  return guarded([&] {
    if (!hp || !out || (!tensors && n_tensors > 0)) throw Err(JAMUN_ERR_INVALID, "null argument");
    // (Conv models of any width and radial size run: outside the compiled-width kernels' envelope on the wide path, jamun_wide.hip;
    // SeparableConv keeps its envelope)
    if (hp->separable && hp->edge_attr_dim != 64) throw Err(JAMUN_ERR_INVALID, "only edge_attr_dim = 64 is supported");
    if (hp->edge_attr_dim < 2) throw Err(JAMUN_ERR_INVALID, "edge_attr_dim must be at least 2 (one bonded and one radial feature)");
    if (hp->mul0 < 1 || hp->mul1 < 0 || hp->n_layers < 0) throw Err(JAMUN_ERR_INVALID, "bad irreps_hidden / n_layers");
    if (hp->separable && ((hp->mul0 + hp->mul1 + 31) / 32 > 5 || (hp->mul1 + 31) / 32 > 2))
      throw Err(JAMUN_ERR_INVALID, "irreps_hidden too wide for the compiled conv tiles (mul0 + mul1 <= 160, mul1 <= 64)");
    if (hp->mul1 == 0) throw Err(JAMUN_ERR_INVALID, "irreps_hidden needs at least one 1e channel (output is 1x1e)");
    if (hp->emb_dim[0] != hp->emb_dim[1])
      throw Err(JAMUN_ERR_INVALID, "atom_type and atom_code embedding dims must match (reference atom_embedding.py:54-56)");
    std::unique_ptr<jamun_model> m(new jamun_model());
    m->hp = *hp;
    for (int i = 0; i < n_tensors; ++i) {
      if (!tensors[i].name || (!tensors[i].data && tensors[i].numel > 0)) throw Err(JAMUN_ERR_INVALID, "tensor table entry with null name/data");
      m->t[tensors[i].name] = std::vector<float>(tensors[i].data, tensors[i].data + tensors[i].numel);
    }
    *out = m.release();
  });
}
void jamun_model_destroy(jamun_model* m) { delete m; }

static void sampler_self_check(const jamun_model* m, float sigma, const jamun_topology* topo, jamun_sampler* s);

int jamun_sampler_create(const jamun_model* m, float sigma, const jamun_topology* topo, const jamun_tuning* tuning, jamun_sampler** out) {
  return guarded([&] {
    if (!m || !topo || !out) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (tuning && (tuning->selfcheck < -1 || tuning->selfcheck > 2)) throw Err(JAMUN_ERR_INVALID, "jamun_tuning.selfcheck must be -1 (off), 0 (default: on), 1 (on) or 2 (on, with an injected fault)");
    std::unique_ptr<jamun_sampler> s = sampler_create_impl(m, sigma, topo, tuning);
    if (!tuning || tuning->selfcheck >= 0) sampler_self_check(m, sigma, topo, s.get());
    *out = s.release();
  });
}

// Create-time self-check: a build whose specialised kernels compute something else than the general ones must not sample.
// The sampler's FIRST forward — on synthetic positions: one random-walk chain per walker, 0.15 nm steps, so that neighbourhoods are as dense
// as a peptide's and the 32-neighbour cap binds on large molecules — is run twice: through the kernels this sampler selected (matrix-formed /
// destination-grouped conv, table or matrix-formed initial projector, f16x3 node update and radial MLP) and through a second, temporary
// sampler restricted to the general kernels (k_conv, k_node_update, k_edge_h: fp32 MFMAs / vector ALUs, no host-planned tiles).  Node
// features after every block and the network output must agree to 2e-5 of the block's largest feature (the parity tests' bound; the f16x3
// kernels sit at 1e-6).  The opt-in reduced-precision mode (f16x1) is checked against its own bound, 2e-2.  SeparableConv has one
// implementation and is not checked; neither is the wide path (jamun_wide.hip): it IS the general path for the models it serves (fp32
// MFMAs / vector ALUs, no host-planned tiles), so it selects no specialised kernel and builds no second sampler.  Cost: one general-kernel forward + the packing of its weights (cfg2: 0.3 s, once per sampler).
static void sampler_self_check(const jamun_model* m, float sigma, const jamun_topology* topo, jamun_sampler* s) {
  if (s->plan.conv_path != CONV_DG) return;  // (the specialised kernels, the initial projector's included, all run on the destination-grouped tile plan)
  jamun_tuning rt{};
  rt.no_dg = rt.no_mf = rt.no_mfi = rt.no_init_v = rt.no_ml = rt.no_tail = 1;
  rt.node_fp32 = rt.edge_h_fp32 = 1;
  rt.selfcheck = -1;
  const std::unique_ptr<jamun_sampler> r = sampler_create_impl(m, sigma, topo, &rt);
  const int N = s->n_atoms;
  std::vector<float> y((size_t)N * 3);
  {
    uint64_t z = 0x9e3779b97f4a7c15ull;
    auto u = [&]() { z = z * 6364136223846793005ull + 1442695040888963407ull; return (float)((z >> 40) & 0xffffff) / 8388608.0f - 1.0f; };  // (-1, 1)
    for (int g = 0; g < topo->n_graphs; ++g) {
      float px = 0.f, py = 0.f, pz = 0.f;
      for (int a = topo->ptr[g]; a < topo->ptr[g + 1]; ++a) {
        float dx, dy, dz, n2;
        do { dx = u(); dy = u(); dz = u(); n2 = dx * dx + dy * dy + dz * dz; } while (n2 < 0.05f || n2 > 1.f);
        const float inv = 0.15f / sqrtf(n2);
        px += dx * inv; py += dy * inv; pz += dz * inv;
        y[(size_t)a * 3] = px; y[(size_t)a * 3 + 1] = py; y[(size_t)a * 3 + 2] = pz;
      }
    }
  }
  DevArena y_mem;
  float* y_dev = y_mem.upload(y);
  if (s->tune.selfcheck == 2 && s->layers.size() > 1) {
    // fault injection (tests): 4 KB of the first hidden layer's weight stream of the SELECTED kernel read as zeros from here on
    float4* w = s->layers[1].dg.wm ? s->layers[1].dg.wm : s->layers[1].dg.wxh ? s->layers[1].dg.wxh : s->layers[1].dg.wx;
    if (w) HIPCHECK(hipMemset(reinterpret_cast<char*>(w) + 64 * 1024, 0, 4096));
  }
  hipStream_t st = nullptr;
  forward(s, y_dev, s->xhat_buf, nullptr, st);
  forward(r.get(), y_dev, r->xhat_buf, nullptr, st);
  HIPCHECK(hipStreamSynchronize(st));
  mf_err_fetch(s, st);
  HIPCHECK(hipStreamSynchronize(st));
  mf_err_check(s);
  const int n_cmp = std::min(N, 16384);  // (rows compared per block: the first 512 tiles — every tile runs the same code)
  std::vector<float> a((size_t)n_cmp * s->XS), b((size_t)n_cmp * s->XS);
  const double tol = s->x1 ? 2e-2 : 2e-5;
  auto compare = [&](const float* da, const float* db, size_t n, const char* what, int layer) {
    HIPCHECK(hipMemcpy(a.data(), da, n * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(b.data(), db, n * sizeof(float), hipMemcpyDeviceToHost));
    double mx = 0, dv = 0;
    bool finite = true;
    for (size_t i = 0; i < n; ++i) {
      finite = finite && std::isfinite(a[i]) && std::isfinite(b[i]);
      mx = std::max(mx, (double)std::fabs(b[i]));
      dv = std::max(dv, (double)std::fabs(a[i] - b[i]));
    }
    if (!finite || dv > tol * std::max(mx, 1e-6)) {
      char msg[320];
      snprintf(msg, sizeof msg, "create-time self-check failed: %s%d of the selected kernels (conv path %d, mode %d, initial projector %d) deviates from the general kernels by %.3g of its largest value (bound %.0e)%s — this build must not sample",
               what, layer, (int)s->plan.conv_path, (int)s->plan.dg_mode, (int)s->plan.init_path, finite ? dv / std::max(mx, 1e-6) : NAN, tol, finite ? "" : " (non-finite values)");
      throw Err(JAMUN_ERR_INVALID, msg);
    }
  };
  for (size_t l = 0; l < s->layers.size(); ++l) compare(s->x[l], r->x[l], (size_t)n_cmp * s->XS, "node features after block ", (int)l);
  compare(s->g, r->g, (size_t)n_cmp * 3, "network output g, block ", (int)s->layers.size());
  if (s->dev.ml_count) { HIPCHECK(hipMemset(s->dev.ml_count, 0, sizeof(unsigned long long))); s->ml_launches = 0; }  // (the check's launches are not the run's)
  // a device memset need not have finished when it returns: create is synchronous and leaves nothing pending, whatever stream comes first
  HIPCHECK(hipDeviceSynchronize());
  s->edges_built = false;
}
void jamun_sampler_destroy(jamun_sampler* s) { delete s; }

int jamun_xhat(jamun_sampler* s, const float* y_dev, float* xhat_dev, void* stream) {
  return guarded([&] {
    if (!s || !y_dev || !xhat_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    mf_err_check(s);
    forward(s, const_cast<float*>(y_dev), xhat_dev, nullptr, (hipStream_t)stream);  // (y is written only with a fused pre-update)
    mf_err_fetch(s, (hipStream_t)stream);
  });
}
int jamun_score(jamun_sampler* s, const float* y_dev, float* score_dev, void* stream) {
  return guarded([&] {
    if (!s || !y_dev || !score_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    mf_err_check(s);
    forward(s, const_cast<float*>(y_dev), nullptr, score_dev, (hipStream_t)stream);
    mf_err_fetch(s, (hipStream_t)stream);
  });
}

int jamun_num_frames(const jamun_mcmc_params* p, int32_t* n_y, int32_t* n_s_baoab, int32_t* n_s_aboba) {
  return guarded([&] {
    check_mcmc(p);
    int ny = saves(p, 0) ? 1 : 0, extra = 0;
    for (int i = 1; i < p->steps; ++i) extra += saves(p, i) ? 1 : 0;
    if (n_y) *n_y = ny + extra;
    if (n_s_baoab) *n_s_baoab = 1 + extra;
    if (n_s_aboba) *n_s_aboba = extra;
  });
}

int jamun_walk_baoab(jamun_sampler* s, float* y, float* v, const jamun_mcmc_params* p, const float* noise,
                     uint64_t seed, float* y_traj, float* score_traj, float* xhat_traj, float* xhat_out, void* stream) {
  return guarded([&] {
    if (!s || !y || !v) throw Err(JAMUN_ERR_INVALID, "null argument");
    check_mcmc(p);
    mf_err_check(s);
    hipStream_t st = (hipStream_t)stream;
    const LangevinConsts k = make_consts(p);
    const int n = s->n_atoms;
    const size_t fr = (size_t)n * 3;
    int fy = 0, fs = 0;
    // The two halves of an iteration run inside the first and the last kernel of the forward (k_geom, k_finalize): one step =
    // the forward's launches and nothing else — and (round 6) the last kernel of iteration i IS the first of iteration i + 1
    // (k_finalize_geom: 20 launches per step instead of 21; jamun_tuning.no_fuse_geom: the two separate kernels).
    // i = 0: initial frame + initial score (_splitting.py:136-155)
    const bool fuse = !s->tune.no_fuse_geom;
    auto make_pre = [&](int i) {
      LangevinPre pre;
      pre.v = v; pre.psi = s->psi; pre.noise = noise ? noise + fr * (size_t)(i - 1) : nullptr; pre.seed = seed; pre.iter = (uint32_t)i; pre.k = k;
      return pre;
    };
    auto make_post = [&](bool sv, int update_v, bool keep_score) {
      LangevinPost post;
      post.psi_out = s->psi; post.v = v; post.update_v = update_v; post.k = k;
      post.y_frame = (y_traj && sv) ? y_traj + fr * fy : nullptr;
      post.xhat_frame = (xhat_traj && sv) ? xhat_traj + fr * fy : nullptr;
      post.score_frame = (score_traj && keep_score) ? score_traj + fr * fs : nullptr;
      return post;
    };
    {
      const bool sv = saves(p, 0);
      const LangevinPost post = make_post(sv, 0, true);
      const LangevinPre pre1 = make_pre(1);
      forward(s, y, s->xhat_buf, s->score_buf, st, LangevinPre(), post, (fuse && p->steps > 1) ? &pre1 : nullptr);
      if (sv) ++fy;
      ++fs;
    }
    for (int i = 1; i < p->steps; ++i) {
      const LangevinPre pre = make_pre(i), pre_next = make_pre(i + 1);
      const bool sv = saves(p, i);
      // scores after the initial one are kept only together with the trajectory (_splitting.py:168-170): without y_traj
      // the caller's score_traj holds ONE frame
      const LangevinPost post = make_post(sv, 1, y_traj && sv);
      forward(s, y, s->xhat_buf, s->score_buf, st, pre, post, (fuse && i + 1 < p->steps) ? &pre_next : nullptr, /*geom_done=*/fuse);
      if (sv) { ++fy; ++fs; }
    }
    if (xhat_out) launch_copy(s->xhat_buf, xhat_out, n * 3, st);  // last forward was evaluated at the final y
    mf_err_fetch(s, st);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_walk_aboba(jamun_sampler* s, float* y, float* v, const jamun_mcmc_params* p, const float* noise,
                     uint64_t seed, float* y_traj, float* score_traj, float* xhat_traj, float* xhat_out, void* stream) {
  return guarded([&] {
    if (!s || !y || !v) throw Err(JAMUN_ERR_INVALID, "null argument");
    check_mcmc(p);
    mf_err_check(s);
    hipStream_t st = (hipStream_t)stream;
    const LangevinConsts k = make_consts(p);
    const int n = s->n_atoms;
    const size_t fr = (size_t)n * 3;
    int fy = 0, fs = 0;
    if (saves(p, 0)) {
      if (y_traj) launch_copy(y, y_traj, n * 3, st);
      if (xhat_traj) forward(s, y, xhat_traj, nullptr, st);
      ++fy;
    }
    for (int i = 1; i < p->steps; ++i) {
      launch_aboba_a(y, v, n, k.half_delta, st);
      forward(s, y, nullptr, s->score_buf, st);
      const bool sv = saves(p, i);
      float* yf = (y_traj && sv) ? y_traj + fr * fy : nullptr;
      float* sf = (score_traj && sv) ? score_traj + fr * fs : nullptr;
      launch_aboba_b(y, v, s->score_buf, noise ? noise + fr * (size_t)(i - 1) : nullptr, seed, (uint32_t)i, n, k, yf, sf, st);
      if (sv) {
        if (xhat_traj) forward(s, y, xhat_traj + fr * fy, nullptr, st);  // one extra forward per saved frame, as the reference
        ++fy; ++fs;
      }
    }
    if (xhat_out) forward(s, y, xhat_out, nullptr, st);
    mf_err_fetch(s, st);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_mean_center(const float* pos, const int32_t* ptr, int32_t n_graphs, float* out, void* stream) {
  return guarded([&] {
    if (!pos || !ptr || !out || n_graphs < 0) throw Err(JAMUN_ERR_INVALID, "bad argument");
    if (n_graphs == 0) return;
    launch_mean_center(pos, ptr, n_graphs, out, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_radius_graph(const float* pos, const int32_t* ptr, int32_t n_graphs, int32_t n_atoms, float r, int32_t stride,
                       int32_t* nbr, int32_t* deg, void* stream) {
  return guarded([&] {
    if (!pos || !ptr || !nbr || !deg || n_graphs < 0 || n_atoms < 0) throw Err(JAMUN_ERR_INVALID, "bad argument");
    if (stride < JAMUN_MAX_NEIGHBORS + 1) throw Err(JAMUN_ERR_INVALID, "stride must be >= 33");
    if (n_graphs == 0) return;
    launch_radius_graph(pos, ptr, n_graphs, r * r, stride, nbr, deg, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_scatter_mean(const float* src, const int32_t* seg_ptr, int32_t n_out, int32_t width, float* out, void* stream) {
  return guarded([&] {
    if (!seg_ptr || !out || n_out < 0 || width < 1) throw Err(JAMUN_ERR_INVALID, "bad argument");
    if (n_out == 0) return;
    launch_scatter_mean(src, seg_ptr, n_out, width, out, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_baoab_pre(float* y, float* v, const float* psi, const float* noise, int32_t n, const jamun_mcmc_params* p,
                    void* stream) {
  return guarded([&] {
    if (!y || !v || !psi || !noise || !p) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (n == 0) return;
    launch_baoab_pre(y, v, psi, noise, 0, 0, n, make_consts(p), (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}
int jamun_baoab_post(float* v, float* psi, const float* score, int32_t n, const jamun_mcmc_params* p, void* stream) {
  return guarded([&] {
    if (!v || !psi || !score || !p) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (n == 0) return;
    launch_baoab_post(v, psi, score, nullptr, nullptr, n, make_consts(p), 1, nullptr, nullptr, nullptr, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_aboba_a(float* y, const float* v, int32_t n, const jamun_mcmc_params* p, void* stream) {
  return guarded([&] {
    if (!y || !v || !p) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (n == 0) return;
    launch_aboba_a(y, v, n, make_consts(p).half_delta, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}
int jamun_aboba_b(float* y, float* v, const float* score, const float* noise, int32_t n, const jamun_mcmc_params* p,
                  void* stream) {
  return guarded([&] {
    if (!y || !v || !score || !noise || !p) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (n == 0) return;
    launch_aboba_b(y, v, score, noise, 0, 0, n, make_consts(p), nullptr, nullptr, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_edge_geometry(const float* pos, int32_t n_atoms, const int64_t* src, const int64_t* dst, int32_t n_edges, float radial_cutoff,
                        int32_t n_basis, float* sh, float* radial, void* stream) {
  return guarded([&] {
    if (!pos || !src || !dst || !sh || !radial || n_edges < 0 || n_atoms < 0) throw Err(JAMUN_ERR_INVALID, "bad argument");
    if (n_basis < 1 || !(radial_cutoff > 0)) throw Err(JAMUN_ERR_INVALID, "n_basis must be >= 1 and radial_cutoff positive");
    if (n_edges == 0) return;
    launch_edge_geometry(pos, (const long long*)src, (const long long*)dst, n_edges, n_atoms, radial_cutoff, n_basis, sh, radial, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_node_linear(const float* x, int32_t n_atoms, int32_t in0, int32_t in1, int32_t out0, int32_t out1, const float* w, int64_t w_numel,
                      float* out, void* stream) {
  return guarded([&] {
    if (!x || !w || !out || n_atoms < 0 || in0 < 0 || in1 < 0 || out0 < 0 || out1 < 0 || in0 + in1 < 1 || out0 + out1 < 1)
      throw Err(JAMUN_ERR_INVALID, "bad argument");
    if (w_numel != (int64_t)in0 * out0 + (int64_t)in1 * out1)
      throw Err(JAMUN_ERR_INVALID, "weight has " + std::to_string(w_numel) + " elements, the irreps need in0*out0 + in1*out1 = " +
                                       std::to_string((int64_t)in0 * out0 + (int64_t)in1 * out1));
    if (n_atoms == 0) return;
    if (launch_node_linear(x, n_atoms, in0, in1, out0, out1, w, out, (hipStream_t)stream) != 0)
      throw Err(JAMUN_ERR_INVALID, "input irreps too wide (8 feature rows must fit 60 KiB of LDS)");
    HIPCHECK(hipGetLastError());
  });
}

int jamun_philox_normal(float* out_dev, int32_t n, uint64_t seed, uint32_t iteration, uint32_t first_atom, void* stream) {
  return guarded([&] {
    if (!out_dev || n < 0) throw Err(JAMUN_ERR_INVALID, "bad argument");
    if (n == 0) return;
    launch_philox_normal(out_dev, n, seed, iteration, first_atom, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_build_edges(jamun_sampler* s, const float* y_dev, void* stream) {
  return guarded([&] {
    if (!s || !y_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    build_edges(s, const_cast<float*>(y_dev), (hipStream_t)stream);  // (y is written only with a fused pre-update)
    HIPCHECK(hipGetLastError());
  });
}

int jamun_conv_block(jamun_sampler* s, int32_t layer, const float* x_in_dev, float* x_out_dev, void* stream) {
  return guarded([&] {
    if (!s || !x_out_dev) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (layer < 0 || layer >= (int)s->layers.size()) throw Err(JAMUN_ERR_INVALID, "layer out of range");
    if (!s->edges_built) throw Err(JAMUN_ERR_INVALID, "no edge table yet: call jamun_build_edges (or a forward) first");
    mf_err_check(s);
    if (layer == 0) {
      if (x_in_dev) throw Err(JAMUN_ERR_INVALID, "block 0 (initial projector) takes the sampler's own noise-scaled atom embedding: pass x_in = NULL");
      run_layer(s, 0, s->x_emb, s->n_emb, x_out_dev, (hipStream_t)stream);
    } else {
      if (!x_in_dev) throw Err(JAMUN_ERR_INVALID, "null x_in");
      if (x_in_dev == x_out_dev) throw Err(JAMUN_ERR_INVALID, "x_in and x_out must not alias (the skip path reads x_in after the conv)");
      run_layer(s, (size_t)layer, x_in_dev, s->XS, x_out_dev, (hipStream_t)stream);
    }
    mf_err_fetch(s, (hipStream_t)stream);
    HIPCHECK(hipGetLastError());
  });
}

int jamun_sampler_stats(jamun_sampler* s, jamun_stats* out, void* stream) {
  return guarded([&] {
    if (!s || !out) throw Err(JAMUN_ERR_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    HIPCHECK(hipMemsetAsync(s->counter, 0, sizeof(unsigned long long), st));
    launch_count_edges(s->deg, s->n_atoms, s->counter, st);
    unsigned long long e = 0;
    HIPCHECK(hipMemcpyAsync(&e, s->counter, sizeof(e), hipMemcpyDeviceToHost, st));
    int mf_flag = 0;
    if (s->dev.mf_err) HIPCHECK(hipMemcpyAsync(&mf_flag, s->dev.mf_err, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    // (k_conv_mf / k_conv_mfi: an ordered pair with more than three edges cannot share one coefficient entry; the host excludes such
    // topologies at create time, the kernels still flag what they see)
    if (mf_flag != 0) {
      if (s->dev.mf_err_host) *s->dev.mf_err_host = mf_flag;
      mf_err_check(s);
    }
    const bool dg = s->plan.conv_path == CONV_DG;
    unsigned long long ml_cnt = 0;
    if (ml_counted(s)) HIPCHECK(hipMemcpy(&ml_cnt, s->dev.ml_count, sizeof(ml_cnt), hipMemcpyDeviceToHost));
    fill_stats_model(s, (int64_t)e, ml_cnt, out);
    out->n_edges = (int64_t)e;
    out->conv_k0 = s->layers.back().p0.K;
    out->conv_k1 = s->layers.back().p1.K;
    out->edge_stride = s->S;
    out->n_slices = dg ? s->plan.segs.n_slabs : s->n_slices;
    out->conv_path = std::max(0, (int)s->plan.conv_path);  // (SeparableConv: reported as 0, like the general kernels)
    out->dg_mode = dg ? (int)s->plan.dg_mode : -1;
    out->init_path = std::max(0, (int)s->plan.init_path);
    out->dg_row_blocks = dg && s->plan.tiles.row_blocks ? 1 : 0;
    out->dg_emu = s->plan.conv_path == CONV_WIDE ? 0 : dg ? (s->x1 ? 2 : s->plan.dg_emu) : -1;  // (the wide path: fp32 MFMAs, jamun_tuning.f16x1 ignored)
    out->n_tail_tiles = s->plan.n_tail_tiles();
    out->n_tail = s->plan.n_tail();
    out->mf_nks = (dg && s->plan.dg_mode == DG_MF) ? s->plan.mf_nks : 0;
    out->ml_window = dg ? s->plan.ml_window : 0;  // (set with DG_ML only)
  });
}

int jamun_sampler_check(jamun_sampler* s, void* stream) {
  return guarded([&] {
    if (!s) throw Err(JAMUN_ERR_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    mf_err_fetch(s, st);
    HIPCHECK(hipStreamSynchronize(st));
    mf_err_check(s);
  });
}

int jamun_profile_enable(jamun_sampler* s, int32_t on) {
  return guarded([&] {
    if (!s) throw Err(JAMUN_ERR_INVALID, "null argument");
    s->prof_mask = on == 1 ? 0xffffffffu : (unsigned)on >> 1;  // 1: every class; otherwise bit (c + 1) selects class c
    s->ev_used.clear();
    s->ev_next = 0;
    for (int& n : s->prof_seen) n = 0;
  });
}

int jamun_profile_sample(jamun_sampler* s, int32_t every) {
  return guarded([&] {
    if (!s || every < 1) throw Err(JAMUN_ERR_INVALID, "every must be >= 1");
    s->prof_every = every;
  });
}

int jamun_profile_read(jamun_sampler* s, double* ms_total, int64_t* launches, void* stream) {
  return guarded([&] {
    if (!s || !ms_total || !launches) throw Err(JAMUN_ERR_INVALID, "null argument");
    HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
    for (int c = 0; c < JAMUN_PROF_NCLASS; ++c) { ms_total[c] = 0; launches[c] = 0; }
    for (auto& u : s->ev_used) {
      float ms = 0;
      HIPCHECK(hipEventElapsedTime(&ms, s->ev_pool[u.second.first], s->ev_pool[u.second.second]));
      ms_total[u.first] += ms;
      launches[u.first] += 1;
    }
    s->ev_used.clear();
    s->ev_next = 0;
  });
}

int jamun_debug_stamps(unsigned long long* out8) {
  return guarded([&] {
    if (!out8) throw Err(JAMUN_ERR_INVALID, "null argument");
    HIPCHECK(hipDeviceSynchronize());
    tprod_print_stamps();
    conv_dg_print_stamps();
    conv_initv_print_stamps();
    conv_mf_print_stamps();
    conv_ml_print_stamps();
    node_print_stamps();
    for (int i = 0; i < 8; ++i) out8[i] = 0;
  });
}

int jamun_debug_live_allocations(int64_t* count, int64_t* bytes) {
  return guarded([&] {
    if (!count || !bytes) throw Err(JAMUN_ERR_INVALID, "null argument");
    *count = DevArena::live_allocs; *bytes = DevArena::live_bytes;
  });
}

int jamun_debug_read(jamun_sampler* s, int32_t what, int32_t layer, float* out, void* stream) {
  return guarded([&] {
    if (!s || !out) throw Err(JAMUN_ERR_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (what == 0) {
      if (layer < 0 || layer >= (int)s->x.size()) throw Err(JAMUN_ERR_INVALID, "layer out of range");
      launch_copy(s->x[layer], out, s->n_atoms * s->XS, st);
    } else if (what == 1) {
      launch_deg_to_float(s->deg, out, s->n_atoms, st);
    } else if (what == 2) {
      launch_copy(s->g, out, s->n_atoms * 3, st);
    } else {
      throw Err(JAMUN_ERR_INVALID, "unknown debug buffer");
    }
    HIPCHECK(hipGetLastError());
  });
}

int jamun_debug_plan_segments(int32_t cus, int32_t ng, int32_t n_k, int32_t n_atoms, int32_t n_tiles, const int32_t* tile_atoms,
                              const int32_t* tile_chunk, int32_t n_chunks, const int64_t* tile_weight, const int8_t* skip, double seg_cost,
                              int32_t* segs_out, int64_t segs_capacity, int32_t* max_segs, int32_t* n_slabs, int32_t* atom_nslab) {
  return guarded([&] {
    if (!max_segs || !n_slabs || !atom_nslab || (n_tiles > 0 && (!tile_atoms || !tile_chunk || !tile_weight)))
      throw Err(JAMUN_ERR_INVALID, "null argument");
    if (cus < 1 || n_atoms < 0 || n_tiles < 0 || n_chunks < 0) throw Err(JAMUN_ERR_INVALID, "bad sizes");
    if ((ng != 1 && ng != 2 && ng != 4 && ng != 8) || (ng > 1 && cus % 8 != 0) || n_k < ng)
      throw Err(JAMUN_ERR_INVALID, "ng must be 1, 2, 4 or 8, with cus % 8 == 0 and n_k >= ng when above 1 (as jamun_sampler_create)");
    if (!(seg_cost >= 0.0 && seg_cost <= 1000.0)) throw Err(JAMUN_ERR_INVALID, "seg_cost out of range [0, 1000]");
    std::vector<int2> t_atoms((size_t)n_tiles);
    std::vector<int> t_chunk((size_t)n_tiles);
    std::vector<int64_t> w((size_t)n_tiles);
    std::vector<char> sk((size_t)n_tiles, 0);
    for (int t = 0; t < n_tiles; ++t) {
      t_atoms[t] = make_int2(tile_atoms[2 * t], tile_atoms[2 * t + 1]);
      if (t_atoms[t].x < 0 || t_atoms[t].y < 1 || t_atoms[t].y > 32 || t_atoms[t].x + t_atoms[t].y > n_atoms) throw Err(JAMUN_ERR_INVALID, "tile atoms out of range");
      t_chunk[t] = tile_chunk[t];
      if (t_chunk[t] < 0 || t_chunk[t] >= n_chunks) throw Err(JAMUN_ERR_INVALID, "tile chunk out of range");
      w[t] = tile_weight[t];
      if (w[t] < 1) throw Err(JAMUN_ERR_INVALID, "tile weights must be >= 1");
      sk[t] = skip ? (char)(skip[t] != 0) : 0;
    }
    // (the sampler's own planner: the same function, only the tile weights come from the caller)
    SegPlan P = plan_segments(cus, ng, n_k, n_atoms, t_atoms, t_chunk, n_chunks, w, skip ? &sk : nullptr, seg_cost);
    *max_segs = P.max_segs;
    *n_slabs = P.n_slabs;
    std::copy(P.atom_nslab.begin(), P.atom_nslab.end(), atom_nslab);
    if (segs_out) {
      if ((int64_t)P.segs.size() * 4 > segs_capacity) throw Err(JAMUN_ERR_INVALID, "segs_out too small: needs cus * max_segs * 8 values");
      std::memcpy(segs_out, P.segs.data(), P.segs.size() * sizeof(int4));
    }
  });
}

int jamun_debug_select_kernels(const jamun_hparams* hp, const jamun_tuning* tuning, const jamun_topology* topo, int32_t cus, int32_t n_uniq,
                               int32_t have_atom_uid, int32_t n_hidden, const int32_t* hidden, const int32_t* layer0, int64_t* out24,
                               int32_t which, int32_t* list, int64_t capacity, int64_t* list_len) {
  return guarded([&] {
    if (!hp || !topo || !layer0 || !out24 || !list_len || (n_hidden > 0 && !hidden)) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (cus < 1 || n_hidden < 0 || topo->n_atoms < 1 || topo->n_graphs < 1) throw Err(JAMUN_ERR_INVALID, "bad sizes");
    const jamun_tuning tn = checked_tuning(tuning);
    PackedLayouts lay;
    for (int l = 0; l < n_hidden; ++l) lay.hidden.push_back({(hidden[l] & 1) != 0, (hidden[l] & 2) != 0, (hidden[l] & 4) != 0});
    lay.tt2 = layer0[0] != 0; lay.tabw = layer0[1] != 0; lay.tab_ut = layer0[2]; lay.wx = layer0[3] != 0; lay.nt0 = layer0[4];
    // (the sampler's own selection: the same functions, only the layout flags come from the caller)
    const TopoHost th = check_topology(*topo);
    const ConvPath base = base_conv_path(*hp, hp->emb_dim[0] + hp->emb_dim[1] + hp->emb_dim[2] + hp->emb_dim[3]);
    const KernelPlan P = select_kernels(*hp, tn, *topo, th, cus, base, lay, n_uniq, have_atom_uid != 0);
    const TilePlan& T = P.tiles;
    const int64_t v[24] = {P.conv_path, P.dg_mode, P.init_path, P.dg_emu, P.dg_RS, th.S, (int64_t)T.atoms.size(), T.span_max, T.row_blocks,
                           (int64_t)P.tail_tiles.size(), (int64_t)P.tail_atom.size(), P.tail_runs, P.init_tail, P.own_init_segs, P.mf_nks, P.ml_window,
                           P.initv_nbuf, P.ng, std::lround(10 * P.seg_cost), P.segs.max_segs, P.segs.n_slabs, conv_model(P, *hp, topo->n_atoms).conv_flop,
                           P.init_segs.max_segs, P.init_segs.n_slabs};
    std::copy(v, v + 24, out24);
    std::vector<int32_t> flat;
    auto int4s = [&](const std::vector<int4>& r) { for (const int4& q : r) flat.insert(flat.end(), {q.x, q.y, q.z, q.w}); };
    switch (which) {
      case -1: break;
      case 0: int4s(P.segs.segs); break;
      case 1: if (P.own_init_segs) int4s(P.init_segs.segs); break;
      case 2: int4s(P.tail_tiles); break;
      case 3: for (size_t t = 0; t < T.atoms.size(); ++t) flat.insert(flat.end(), {T.atoms[t].x, T.atoms[t].y, T.span[t].x, T.span[t].y}); break;
      case 4: flat = P.segs.atom_nslab; break;
      case 5: if (P.own_init_segs) flat = P.init_segs.atom_nslab; break;
      case 6: flat = T.chunk; break;
      default: throw Err(JAMUN_ERR_INVALID, "unknown work list");
    }
    *list_len = (int64_t)flat.size();
    if (!list || flat.empty()) return;
    if ((int64_t)flat.size() > capacity) throw Err(JAMUN_ERR_INVALID, "list too small: needs list_len values");
    std::copy(flat.begin(), flat.end(), list);
  });
}

int jamun_debug_segments(jamun_sampler* s, int32_t which, int32_t* out, int64_t capacity, int32_t* info) {
  return guarded([&] {
    if (!s || !info) throw Err(JAMUN_ERR_INVALID, "null argument");
    if (s->plan.conv_path != CONV_DG) throw Err(JAMUN_ERR_INVALID, "the sampler has no destination-grouped plan (jamun_tuning.no_dg)");
    const void* src = nullptr;
    int64_t n = 0;
    const KernelPlan& P = s->plan;
    const SegPlan& L = which == 1 ? P.init_segs : P.segs;
    const bool have = which != 1 || P.own_init_segs;  // (without lists of its own the initial projector runs list 0: nothing to report)
    switch (which) {
      case 0: src = s->dev.segs; n = (int64_t)L.segs.size() * 4; break;
      case 1: if (have) { src = s->dev.init_segs; n = (int64_t)L.segs.size() * 4; } break;
      case 2: src = s->dev.tail_tiles; n = (int64_t)P.n_tail_tiles() * 4; break;
      case 3: n = (int64_t)P.n_tiles() * 4; break;
      case 4: src = s->dev.atom_nslab; n = s->n_atoms; break;
      case 5: if (P.own_init_segs) { src = s->dev.init_atom_nslab; n = s->n_atoms; } break;
      default: throw Err(JAMUN_ERR_INVALID, "unknown work list");
    }
    const int32_t v[9] = {(int32_t)n, s->cus, have ? L.max_segs : 0, have ? L.n_slabs : 0, P.ng, s->hp.edge_attr_dim + 1, P.n_tiles(), (int32_t)std::lround(10 * P.seg_cost), P.tail_runs};
    std::copy(v, v + 9, info);
    if (!out || n == 0) return;
    if (n > capacity) throw Err(JAMUN_ERR_INVALID, "out too small: needs info[0] values");
    if (which == 3) {  // {first atom, atoms, first source row, end of the source rows} per tile
      std::vector<int2> a((size_t)P.n_tiles()), sp((size_t)P.n_tiles());
      HIPCHECK(hipMemcpy(a.data(), s->dev.tile_atoms, a.size() * sizeof(int2), hipMemcpyDeviceToHost));
      HIPCHECK(hipMemcpy(sp.data(), s->dev.tile_span, sp.size() * sizeof(int2), hipMemcpyDeviceToHost));
      for (size_t t = 0; t < a.size(); ++t) {
        out[4 * t] = a[t].x; out[4 * t + 1] = a[t].y; out[4 * t + 2] = sp[t].x; out[4 * t + 3] = sp[t].y;
      }
      return;
    }
    HIPCHECK(hipMemcpy(out, src, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
