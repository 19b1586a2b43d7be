// jamun_host.h — host-only declarations shared by jamun_pack.cpp (weight packing), jamun_plan.cpp (tile / work-list planning and
// kernel selection), jamun_api.cpp (sampler create, dispatch, the C ABI), jamun_frames.cpp (the C entries on frames) and jamun_denoise.cpp
// (the C entries of the denoising evaluation).  Not included
// by any .hip file.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/jamun_hip.h"
#include "jamun_internal.h"

struct Err : std::runtime_error {
  int code;
  Err(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIPCHECK(expr)                                                                                 \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess) throw Err(JAMUN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// The calling thread's last error (jamun_last_error) and the wrapper every C entry runs its body in: an exception becomes its code and
// leaves its text in the slot.  One definition for every host file; the library does not export it.
__attribute__((visibility("hidden"))) inline thread_local std::string jamun_error_slot;

template <typename F>
int guarded(F&& f) {
  try {
    f();
    return JAMUN_OK;
  } catch (const Err& e) {
    jamun_error_slot = e.what();
    return e.code;
  } catch (const std::exception& e) {
    jamun_error_slot = e.what();
    return JAMUN_ERR_INVALID;
  }
}

// Owner of device (and pinned host) memory: every allocation it hands out is recorded and freed by clear() / the destructor, so a throw
// anywhere in sampler create gives back what was uploaded so far.  Structs keep plain T* fields into it.  live_allocs / live_bytes count
// what all arenas of the process hold (jamun_debug_live_allocations).
class DevArena {
  struct Block { void* p; size_t bytes; bool pinned; };
  std::vector<Block> blocks_;
  void* take(size_t bytes, bool pinned) {
    blocks_.reserve(blocks_.size() + 1);  // (so that recording the block cannot throw once it exists)
    void* p = nullptr;
    HIPCHECK(pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes));
    blocks_.push_back({p, bytes, pinned});
    ++live_allocs; live_bytes += (int64_t)bytes;
    return p;
  }

 public:
  static inline std::atomic<int64_t> live_allocs{0}, live_bytes{0};
  DevArena() = default;
  DevArena(const DevArena&) = delete;
  DevArena& operator=(const DevArena&) = delete;
  ~DevArena() { clear(); }
  template <typename T> T* alloc(size_t n) { return (T*)take(std::max<size_t>(n, 1) * sizeof(T), false); }
  template <typename T> T* pinned(size_t n) { return (T*)take(std::max<size_t>(n, 1) * sizeof(T), true); }
  template <typename T> T* zeroed(size_t n) { T* p = alloc<T>(n); HIPCHECK(hipMemset(p, 0, std::max<size_t>(n, 1) * sizeof(T))); return p; }
  template <typename T> T* upload(const std::vector<T>& v) {
    T* p = alloc<T>(v.size());
    if (!v.empty()) HIPCHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
  }
  void clear() {
    for (const Block& b : blocks_) {
      b.pinned ? hipHostFree(b.p) : hipFree(b.p);
      --live_allocs; live_bytes -= (int64_t)b.bytes;
    }
    blocks_.clear();
  }
};

struct jamun_model {
  jamun_hparams hp;
  std::map<std::string, std::vector<float>> t;
  const std::vector<float>& get(const std::string& name, int64_t numel = -1) const {
    auto it = t.find(name);
    if (it == t.end()) throw Err(JAMUN_ERR_MISSING, "missing checkpoint tensor: " + name);
    if (numel >= 0 && (int64_t)it->second.size() != numel)
      throw Err(JAMUN_ERR_INVALID, "tensor " + name + " has " + std::to_string(it->second.size()) +
                                       " elements, expected " + std::to_string(numel));
    return it->second;
  }
};

// ---- packed weights of one layer (jamun_pack.cpp) ------------------------------------------------
struct ConvProblemDev {
  float4* wpack = nullptr;
  int4* chunks = nullptr;
  int* slice_ptr = nullptr;
  int4* ublk = nullptr;
  int* lane_xoff = nullptr;
  int planes = 0, nt = 0, xw = 0;
  int64_t K = 0;  // padded contraction depth
};
struct DgDev {
  float4 *wx = nullptr, *wd = nullptr, *wv = nullptr, *wt = nullptr;  // null: the layer cannot use jamun_conv_dg.hip
  float4* wxh = nullptr;  // f16x3 contraction: hi / lo planes of the scaled weights, one stream per (hidden unit, matrix wave)
  float4* wth = nullptr;  // f16x3 T pre-pass: [k][8 groups of 16 inputs][hi, lo][64 lanes], A operand (lane (w', hh): inputs 16 g + 8 hh + j)
  float4* wm = nullptr;   // jamun_conv_mf.hip: [k][4 matrix waves][40 blocks], K index permuted to the forming MFMA's accumulator layout
  int sB = 0, sBt = 0, sTw = 0;
  float hmax2 = 2.f;
  // f16x3 balancing (build_layer): gx [216] 2^e_u per feature element (layout of a feature row), gT [128] the T pre-pass's input factors,
  // cf0 [160] / cf1 [32] / cfT [32] the inverse column scales of the scalar / vector outputs / T
  float *gx = nullptr, *gT = nullptr, *cf0 = nullptr, *cf1 = nullptr, *cfT = nullptr;
  float4* wmt = nullptr;   // tail tiles (k_tail_contract): vector-output weights [k][24 blocks] under one column scale
  float* cf1t = nullptr;   // ... its inverse [32]
};
struct SepDev {
  float4* w2b = nullptr;  // null: not a SeparableConv layer
  float *cfw = nullptr, *bias = nullptr, *wl0 = nullptr, *wl1 = nullptr;
  int n0 = 0, n1 = 0, sH = 0;
};
struct LayerDev {
  ConvProblemDev p0, p1;
  DgDev dg;
  SepDev sep;
  std::vector<float> w1r_h, cmask_h;  // radial MLP first layer (uploaded for all layers together: jamun_sampler::w1r_all)
  int tt_U = 0;  // distinct embedding rows of the tables below
  float* tt2 = nullptr;  // the same table re-laid for k_conv_init_v: [k][U][192]
  float4* tabw = nullptr;  // ... and scaled by 2^tab_sB, split hi + lo, as MFMA B fragments for k_conv_mfi (U <= 32): [k][24 blocks][64 lanes]
  int tab_sB = 0, tab_ut = 0;
  // k_conv_mfx (initial projector formed from the feature rows; batches with more than 32 distinct embedding rows)
  float4* wx = nullptr;                  // [k][48 blocks] balanced, split weights (MfxArgs::wx)
  unsigned *xph = nullptr, *xpl = nullptr;  // the embedding rows times channel factors and 2^x_sX, split, two atoms per word
  int x_sX = 0;
  float *xcf0 = nullptr, *xcf1 = nullptr;
  float4 *wcat0 = nullptr, *wcat1 = nullptr;  // node update: [W_self ; W_skip] as MFMA fragments
  int K0p = 0, K1p = 0;
  float4 *wh0 = nullptr, *wh1 = nullptr;      // ... and balanced per row / column, split hi + lo for the f16x3 kernel (jamun_node.hip)
  int K0h = 0, K1h = 0;
  float *kga0 = nullptr, *kga1 = nullptr, *kgx = nullptr, *cg0 = nullptr, *cg1 = nullptr;  // its row (input) / column (output) powers of two
  float* mix = nullptr;
  float4 *wn0 = nullptr, *wn1 = nullptr;  // wide path (k_node_lin_wide): [W_self ; W_skip] with the K order of NodeWideArgs
  int K0w = 0, K1w = 0;
  int in0 = 0, in1 = 0, XSin = 0;
  int64_t tp_numel = 0;
};

// ---- jamun_pack.cpp -----------------------------------------------------------------------------
std::vector<double> noise_mlp(const jamun_model& m, const std::string& prefix, int k, double c_noise);
struct InBlock { int mul, l, xoff, ch0; };
// (mem owns the layer's buffers; dg_mem those of L.dg, the tile plan's weights, which create releases early when the plan is not selected)
LayerDev build_layer(DevArena& mem, DevArena& dg_mem, const jamun_model& m, const std::string& prefix, const std::vector<InBlock>& in_blocks,
                     const std::vector<double>& s_in, int n_slices,
                     const std::vector<float>* uniq_rows = nullptr, int row_len = 0, bool pack_dg = false,
                     const std::vector<float>* all_rows = nullptr, bool wide = false);

// The conv kernel family of the hidden layers and of the initial projector.  The enumerators carry the numbers jamun_stats documents for
// conv_path / init_path (include/jamun_hip.h); SeparableConv has enumerators of its own here and is reported as 0 (jamun_sampler_stats).
enum ConvPath {
  CONV_GENERAL = 0,  // k_conv (jamun_conv.hip)
  CONV_DG = 2,       // destination-grouped, on host-planned tiles: k_conv_dg / k_conv_mf / k_conv_ml by KernelPlan::dg_mode
  CONV_WIDE = 3,     // k_conv_wide (jamun_wide.hip): a Conv model outside the envelope of the compiled-width kernels
  CONV_SEP = -1      // SeparableConv (jamun_sepconv.hip)
};
enum InitPath {
  INIT_GENERAL = 0,
  INIT_V = 2,    // k_conv_init_v (tiles / segments of the dg kernel)
  INIT_MFI = 3,  // k_conv_mfi (DG_MF tiles, at most 32 distinct embedding rows)
  INIT_MFX = 4,  // k_conv_mfx (DG_MF tiles, any number of distinct rows: formed from the feature rows)
  INIT_MLX = 5,  // k_conv_mlx (DG_ML tiles: large spans)
  INIT_WIDE = 6,
  INIT_SEP = -1
};
// The hidden-layer kernel of CONV_DG.  jamun_stats.dg_mode publishes these numbers; DgArgs::alt receives those of the k_conv_dg variants.
enum DgMode {
  DG_RESIDENT = 0,  // k_conv_dg: two phases per hidden unit, source rows resident in LDS (spans up to ~80 rows)
  DG_ALT = 1,       // k_conv_dg: alternating residency (molecules above that, up to ~176 atoms)
  DG_SINGLE = 2,    // k_conv_dg: single phase with double-buffered A tiles (spans up to ~52 rows)
  DG_SINGLE_Y = 3,  // k_conv_dg: single phase with a double-buffered X tile and one Y tile (spans up to ~73 rows)
  DG_MF = 4,        // k_conv_mf (+ tail tiles): A operand formed on the matrix cores, spans within one K = 64 window (62 rows)
  DG_ML = 5         // k_conv_ml: its two-pass, block-sparse variant for spans of 63..167 rows
};
inline bool matrix_formed(DgMode m) { return m == DG_MF || m == DG_ML; }
// which plans at hand the trial of k_conv_mf / of k_conv_ml may replace (select_kernels)
inline bool mf_may_replace(DgMode m) { return m == DG_RESIDENT || m == DG_SINGLE || m == DG_SINGLE_Y; }
inline bool ml_may_replace(DgMode m) { return m == DG_RESIDENT || m == DG_ALT || m == DG_SINGLE_Y; }

// ---- what jamun_plan.cpp decides ---------------------------------------------------------------------
struct SegPlan {
  std::vector<int4> segs;  // [cus][max_segs][2]
  int max_segs = 1, n_slabs = 1;
  std::vector<int> atom_nslab;
};
struct TilePlan {
  std::vector<int2> atoms, span;  // per tile: {first destination atom, atoms}, {lo, hi} source atoms
  std::vector<int> chunk;         // ... and its destination chunk (tiles of one chunk number their partial slabs jointly)
  int n_chunks = 0, span_max = 0;
  bool row_blocks = false;        // a molecule's sources were cut into row blocks
};
// What select_kernels decides: which kernels run — jamun_stats reports the numbers — and, for CONV_DG, the tiles and work lists they run
// on.  A sampler keeps the plan it was created with, unmodified; dispatch, the stats and jamun_debug_segments read it.  Below init_path the
// fields are meaningful for CONV_DG only.
struct KernelPlan {
  ConvPath conv_path = CONV_GENERAL;
  InitPath init_path = INIT_GENERAL;
  DgMode dg_mode = DG_RESIDENT;
  int dg_emu = 1;  // 1: f16x3 contraction (three f16 MFMAs per fp32 product); 0 (jamun_tuning.dg_fp32): v_mfma_f32_32x32x2_f32
  int dg_RS = 0;   // source rows of a tile in LDS
  TilePlan tiles;
  int ng = 1;             // k-slices over XCD groups and ...
  double seg_cost = 0.0;  // ... the cost of a segment, in items, the work lists were cut with
  SegPlan segs, init_segs;     // work lists of the hidden layers; of the initial projector when it keeps lists of its own (own_init_segs)
  bool own_init_segs = false, init_tail = false;
  std::vector<int4> tail_tiles;  // tail tiles (DG_MF): records, destinations, runs of hidden units, bytes of the parked operands
  std::vector<int> tail_atom;
  int tail_runs = 0;
  size_t tail_P_bytes = 0;
  int mf_nks = 4;      // forming K-steps of k_conv_mf (3: every whole tile's sources lie in the first 48 rows of its window)
  int ml_window = 0;   // DG_ML: source rows of the instantiation (96, 128, 168)
  int initv_nbuf = 2;  // INIT_V: row buffers of k_conv_init_v in LDS
  int n_tiles() const { return (int)tiles.atoms.size(); }
  int n_tail_tiles() const { return (int)tail_tiles.size(); }
  int n_tail() const { return (int)tail_atom.size(); }
};
// The device arrays uploaded from a CONV_DG plan (upload_plan), and the buffers sized by it
struct PlanDev {
  int2 *tile_atoms = nullptr, *tile_span = nullptr;
  int4 *segs = nullptr, *init_segs = nullptr;  // segment records with their tile's descriptor (init_segs: KernelPlan::own_init_segs)
  int *atom_nslab = nullptr, *init_atom_nslab = nullptr;
  // tail tiles (tiles with few destinations): formed with the hidden unit in the column index and contracted 32 gathered destinations at a
  // time (k_tail_form / k_tail_contract) instead of as whole tiles of k_conv_mf
  int4* tail_tiles = nullptr;
  int* tail_atom = nullptr;
  float* tail_scale = nullptr;
  float4* tail_P = nullptr;
  float* T = nullptr;  // [n_k][n_atoms][32] pre-pass product of a hidden layer (k_tprod), reused by every layer
  int tstride = 0;     // matrix-formed kernels: T is [n_k][32][tstride], transposed
  unsigned long long* ml_count = nullptr;  // v_mfma_f32_32x32x16_f16 executed by k_conv_ml since create (depends on the occupied source blocks)
  int* mf_err = nullptr;       // device flag of the matrix-formed kernels
  int* mf_err_host = nullptr;  // pinned copy, refreshed behind every entry point that ran a forward (mf_err_fetch / mf_err_check)
};


struct jamun_sampler {
  DevArena mem, dg_mem;  // every device buffer below (dg_mem: LayerDev::dg); declared first: freed last, after the event pool
  jamun_hparams hp;
  jamun_tuning tune{};  // kernel-selection switches of jamun_sampler_create (all zero: defaults)
  float sigma = 0;
  int n_atoms = 0, n_graphs = 0, n_pad = 0, S = 0, n_slices = 8;
  int XS = 0, n_emb = 0;
  float c_in = 0, c_skip = 0, c_out = 0, r_cut = 0, r2 = 0, rb_step = 0;
  // static device data
  int *ptr = nullptr, *bond_in_ptr = nullptr, *bond_in_src = nullptr;
  int n_tiles = 0;
  KernelPlan plan;  // which kernels run and on which tiles and work lists (select_kernels); not modified after create
  PlanDev dev;      // ... and what upload_plan put on the device for them
  int* atom_uid = nullptr;  // [n_atoms] index of the atom's distinct (scaled) embedding row
  float* sep_D = nullptr;   // SeparableConv: [n_atoms][K0 + 3 K1] per-destination sums of the layer at hand
  int cus = 1;
  int x1 = 0;  // 1: reduced-precision hidden-layer conv (jamun_tuning.f16x1) — honoured by the matrix-formed kernels only; stats report dg_emu 2
  int64_t ml_launches = 0;  // launches of k_conv_ml behind PlanDev::ml_count
  int n_uniq = 0;  // distinct (noise-scaled) embedding rows of the batch
  float *x_emb = nullptr, *mu = nullptr;
  float *z0 = nullptr, *z1 = nullptr;  // CONV_WIDE: node-update operands (NodeWideArgs::z0 / z1)
  std::vector<LayerDev> layers;
  float *w_gate = nullptr, *w_vec = nullptr, *w_out = nullptr;
  // work buffers
  float *w1r_all = nullptr, *cmask_all = nullptr;  // [layers][64][32], [layers][2][64]
  float4* w1h_all = nullptr;                        // k_edge_h16: [layers][2 k-tiles][2 K-steps][hi, lo][64 lanes]
  float* w1isc_all = nullptr;                       // [layers] 2^-(14 + sW)
  size_t h_stride = 0, h_kstride = 0;  // per layer: [65 hidden rows][h_kstride edge slots]
  bool h_batched = false, edges_built = false;
  float *yc = nullptr, *h = nullptr, *partial0 = nullptr, *partial1 = nullptr, *g = nullptr, *tmp = nullptr;
  float *xhat_buf = nullptr, *score_buf = nullptr, *psi = nullptr;
  int *deg = nullptr, *esrc = nullptr;
  int* epair = nullptr;  // k_geom's pair table (jamun_internal.h: JAMUN_EP_*), one word per edge slot
  float4* egeo = nullptr;
  std::vector<float*> x;  // per block output [n_atoms][XS]
  unsigned long long* counter = nullptr;
  int64_t flop_ref_per_edge = 0, flop_exec = 0;
  // optional per-kernel-class timing with HIP events on the launch stream (jamun_profile_*)
  unsigned prof_mask = 0;  // bit c: record HIP events around launches of profile class c
  int prof_every = 1;      // ... around every prof_every-th launch of the class (jamun_profile_sample)
  int prof_seen[JAMUN_PROF_NCLASS] = {0};
  std::vector<hipEvent_t> ev_pool;
  std::vector<std::pair<int, std::pair<int, int>>> ev_used;  // (class, (begin, end))
  size_t ev_next = 0;

  ~jamun_sampler() { for (hipEvent_t e : ev_pool) hipEventDestroy(e); }
};

void pack_head(const jamun_model& m, jamun_sampler* s);  // w_gate / w_vec / w_out
void pack_edge_h16(jamun_sampler* s);                    // w1h_all / w1isc_all from the layers' w1r_h

// ---- jamun_plan.cpp -----------------------------------------------------------------------------
void plan_tiles(const int32_t* ptr, const std::vector<int>& graph_of, int N, int cap, std::vector<int2>& t_atoms,
                std::vector<int2>& t_span, std::vector<int>& t_chunk, int& n_chunks, int& span_max, bool& row_blocks);
SegPlan plan_segments(int cus, int ng, int n_k, int N, const std::vector<int2>& t_atoms, const std::vector<int>& t_chunk, int n_chunks,
                      const std::vector<int64_t>& tile_weight, const std::vector<char>* skip = nullptr, double seg_cost = 0.0);
ConvPath base_conv_path(const jamun_hparams& hp, int n_emb);
// What check_topology derives from a topology on the host: walker of every atom; bonded edges by destination (CSR: pointers, sources);
// atoms of the largest walker; the edge stride (32 radial slots + the largest bonded in-degree, at least 1)
struct TopoHost { std::vector<int> graph_of, bip, bis; int nmax = 0, S = 1; };
TopoHost check_topology(const jamun_topology& topo);
// Which weight layouts packing produced (jamun_pack.cpp), as far as kernel selection asks: plain flags, filled from the sampler's layers
struct PackedLayouts {
  struct Hidden { bool dg, mf, tail; };  // a hidden layer's weights for k_conv_dg (DgDev::wx), k_conv_mf / k_conv_ml (wm), the tail tiles (wmt)
  std::vector<Hidden> hidden;
  bool tt2 = false, tabw = false, wx = false;  // initial projector: tables of k_conv_init_v / k_conv_mfi, weights of k_conv_mfx / k_conv_mlx
  int tab_ut = 0, nt0 = 0;                     // ... LayerDev::tab_ut, p0.nt
};
KernelPlan select_kernels(const jamun_hparams& hp, const jamun_tuning& tn, const jamun_topology& topo, const TopoHost& th, int cus, ConvPath base,
                          const PackedLayouts& lay, int n_uniq, bool have_atom_uid);
// FLOP and byte constants of the hidden-layer kernels of a CONV_DG plan, per launch: the matrix-core FLOPs of the conv kernel (tail tiles run
// in their own kernels), of the T pre-pass, and the bytes of the weight stream
struct ConvModel { int64_t conv_flop = 0, tprod_flop = 0, weight_bytes = 0; };
ConvModel conv_model(const KernelPlan& plan, const jamun_hparams& hp, int n_atoms);
