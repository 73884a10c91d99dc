// lsm_host.hip -- the host side of the C ABI in include/lsm_rollout.h: the handle (lsm_env), the
// choice of a step kernel for a configuration (choose_kernel over lsm_kernels.h's table), table
// upload with its small device kernels, the per-step launch and the lsm_host_* exports. The step
// kernels' device code is lsm_rollout.hip's; both sides share lsm_params.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lsm_rollout.h"
#include "lsm_kernels.h"
#include "lsm_params.h"
#include "lsm_rk45.h"
#include "lsm_scenario.h"

namespace lsm {

// One thread per bounds block: min / max over the nodes its cells interpolate (cells
// [b B, (b + 1) B) per dim -> nodes [b B, (b + 1) B] clipped, wrapped on periodic dims),
// widened by 4e-6 max|v|: the fp32 sum of 2^d weighted corners stays within ~20 ulp of
// max|v| of the exact convex combination, so an interpolated value never leaves the bounds.
__global__ void bounds_kernel(const float* values, float2* bnd, TableDev T, int nblocks) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblocks) return;
  const int B = 1 << T.bshift;
  int lo[5], cnt[5];
  int rem = b;
  for (int d = T.ndim - 1; d >= 0; --d) {
    const int ncell = T.periodic[d] ? T.n[d] : T.n[d] - 1;
    const int nb = (ncell + B - 1) / B;
    const int bd = rem % nb;
    rem /= nb;
    lo[d] = bd * B;
    const int hi_cell = min(lo[d] + B, ncell);   // cells [lo, hi_cell)
    cnt[d] = hi_cell - lo[d] + 1;                // nodes lo .. hi_cell
  }
  float mn = INFINITY, mx = -INFINITY;
  int idx[5] = {0, 0, 0, 0, 0};
  for (;;) {
    int64_t node = 0;
    for (int d = 0; d < T.ndim; ++d) {
      int i = lo[d] + idx[d];
      if (T.periodic[d] && i >= T.n[d]) i -= T.n[d];
      node = node * T.n[d] + i;
    }
    const float v = values[node];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
    int d = T.ndim - 1;
    while (d >= 0 && ++idx[d] == cnt[d]) idx[d--] = 0;
    if (d < 0) break;
  }
  const float m = 4.0e-6f * fmaxf(fabsf(mn), fabsf(mx));
  bnd[b] = make_float2(mn - m, mx + m);
}

// grid_pos's reciprocal path against the division for every float32 y in [-neg, pos] (bit patterns
// 0 .. pos_bits and the sign-flipped 0 .. neg_bits): bad = 1 on any difference (NaN == NaN).
__global__ void mdiv_check_kernel(float sp, float rsp, uint32_t pos_bits, uint32_t neg_bits, int* bad) {
  const uint64_t n = (uint64_t)pos_bits + 1 + (uint64_t)neg_bits + 1;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t b = i <= pos_bits ? (uint32_t)i : 0x80000000u | (uint32_t)(i - pos_bits - 1);
    const float y = __uint_as_float(b);
    const float a = grid_pos(y, sp, rsp, 0), c = grid_pos(y, sp, rsp, 1);
    if (__float_as_uint(a) != __float_as_uint(c) && !(a != a && c != c)) *bad = 1;
  }
}

// Expand a node table into the cell-corner layout (one thread per (cell, corner)).
__global__ void expand_cells_kernel(const float* values, const float4* grads, float* cells, float4* gcells,
                                    TableDev T, int64_t n_cells) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int nc = 1 << T.ndim;
  if (t >= n_cells * nc) return;
  const int64_t cell = t / nc;
  const int c = (int)(t - cell * nc);
  int64_t rem = cell, node = 0, nstride = 1;
  int idx[5];
  for (int d = T.ndim - 1; d >= 0; --d) {
    const int ncd = T.periodic[d] ? T.n[d] : T.n[d] - 1;
    idx[d] = (int)(rem % ncd);
    rem /= ncd;
  }
  for (int d = T.ndim - 1; d >= 0; --d) {
    const int bit = (c >> (T.ndim - 1 - d)) & 1;
    int i = idx[d] + bit;
    if (T.periodic[d] && i >= T.n[d]) i -= T.n[d];
    node += (int64_t)i * nstride;
    nstride *= T.n[d];
  }
  cells[t] = values[node];
  if (grads)
    for (int q = 0; q < T.gw; ++q) gcells[t * T.gw + q] = grads[node * T.gw + q];
}

// A new value table (a new HjDataHandle): every env's separation chain starts empty.
__global__ void sep_clear_kernel(float4* rec, uint32_t rec_stride16, int n_envs, uint32_t sep_off) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs) return;
  double* sep = (double*)((unsigned char*)(rec + (size_t)env * rec_stride16) + sep_off);
  sep[0] = 0.0;
  sep[1] = 0.0;
}

// env k's MT19937: np.random.seed(seed + 1000 * (env_offset + k))
__global__ void seed_kernel(uint32_t* mt, int n_envs, int64_t seed, int64_t env_offset) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n_envs) return;
  const uint32_t s = (uint32_t)(seed + 1000 * (env_offset + env));
  uint32_t* key = mt + (size_t)env * MT_WORDS;
  mt_seed(s, key, 1);
  key[MT_N] = MT_N;
}

}  // namespace lsm

// ====================================================================================
// C ABI
// ====================================================================================
using namespace lsm;

// ---- the kernel table (lsm_kernels.h) and the choice of a row -----------------------------------
enum KernelFamily { K_WAVE, K_TEAM, K_BLOCK };

struct KernelRow {
  int family, dyn, nt;
  int sub;           // K_WAVE: lanes per env, K_TEAM: envs per workgroup, K_BLOCK: 0
  bool nis1, rext;   // as instantiated (K_WAVE: one kernel for all, false; K_TEAM: nis1 always)
  lsm_launch_fn launch;
  const char* name;
};

#define LSM_ROW_W(d, lpe, nt) \
  {K_WAVE, d, nt, lpe, false, false, &launch_t<d, lpe, nt>, "rollout_kernel<" #d ", " #lpe ", " #nt ">"},
#define LSM_ROW_T(d, nt, g, rext) \
  {K_TEAM, d, nt, g, true, rext, &launch_team_t<d, nt, g, rext>, "rollout_team_kernel<" #d ", " #nt ", " #g ", " #rext ">"},
#define LSM_ROW_B(d, nt, nis1, rext) \
  {K_BLOCK, d, nt, 0, nis1, rext, &launch_block_t<d, nt, nis1, rext>, "rollout_block_kernel<" #d ", " #nt ", " #nis1 ", " #rext ">"},
static const KernelRow kernel_table[] = {LSM_KERNELS(LSM_ROW_W, LSM_ROW_T, LSM_ROW_B)};

static const KernelRow* find_kernel(int family, int dyn, int nt, int sub, bool nis1, bool rext) {
  for (const KernelRow& r : kernel_table)
    if (r.family == family && r.dyn == dyn && r.nt == nt && r.sub == sub && r.nis1 == nis1 && r.rext == rext)
      return &r;
  return nullptr;
}

// What lsm_create_select derives from (lsm_config, lsm_kernel_select) before it allocates anything.
struct KernelChoice {
  const KernelRow* kernel;   // the row launch() calls and lsm_kernel_name() names
  lsm_kernel_select sel;     // the select block with NULL's defaults filled in (tests, A/B runs)
  int lpe;      // lanes per env: 64 (one env per wave), 32 or 16 (2 or 4 envs per wave)
  bool block;   // workgroup-per-env kernel (N > 32 or E > 64, or sel.workgroup_per_env)
  int team;     // envs per workgroup of the team kernel (lsm_team.h); 0 = rollout_kernel
  bool lean;    // the team kernel's lean LDS layout (airtaxi, N % 4 == 0, E % 4 == 0)
  bool rext;    // KParams::rext: optional reward terms or the shared reward are on
};

// Validate the arguments and pick the kernel: a pure function of its inputs (no handle, no HIP call;
// lsm_kernel_name_for exports it). 1 and *err = the refusal, else 0 and *out.
static int choose_kernel(const lsm_config* cfg, const lsm_kernel_select* sel, KernelChoice* out, std::string* err) {
  auto refuse = [&](const char* msg) { *err = msg; return 1; };
  KernelChoice k;
  if (sel) {
    k.sel = *sel;
  } else {
    memset(&k.sel, 0, sizeof(k.sel));
    k.sel.team = -1;
    k.sel.lean = -1;
    k.sel.filter_search = -1;
  }
  {
    const lsm_kernel_select& s = k.sel;
    if (s.workgroup_per_env != 0 && s.workgroup_per_env != 1) return refuse("kernel select: workgroup_per_env must be 0 or 1");
    if (s.generic != 0 && s.generic != 1) return refuse("kernel select: generic must be 0 or 1");
    if (s.lanes_per_env != 0 && s.lanes_per_env != 16 && s.lanes_per_env != 32 && s.lanes_per_env != 64)
      return refuse("kernel select: lanes_per_env must be 0, 16, 32 or 64");
    if (s.team != -1 && s.team != 0 && s.team != 2 && s.team != 4 && s.team != 8)
      return refuse("kernel select: team must be -1, 0, 2, 4 or 8");
    if (s.lean < -1 || s.lean > 1) return refuse("kernel select: lean must be -1, 0 or 1");
    if (s.filter_search < -1 || s.filter_search > 1) return refuse("kernel select: filter_search must be -1, 0 or 1");
    if (s.bounds_shift < 0 || s.bounds_shift > 4) return refuse("kernel select: bounds_shift must be in [0, 4]");
  }
  const int N = cfg->num_agents, L = cfg->num_landmarks;
  if (cfg->dynamics != LSM_DOUBLE_INTEGRATOR && cfg->dynamics != LSM_AIRTAXI)
    return refuse("dynamics must be LSM_DOUBLE_INTEGRATOR or LSM_AIRTAXI");
  if (N < 2 || N > BMAXN) return refuse("num_agents must be in [2, 64]");
  if (L < (cfg->scenario == LSM_SCENARIO_TRAIN ? 2 : 1) || L > MAX_L)
    return refuse("num_landmarks must be in [2, 8] (the training scenario asserts > 1, utils.py:31; "
                  "layout scenarios: [1, 8])");
  if (N * (1 + L) > BMAXE) return refuse("N * (1 + L) must be <= 256");
  if (N * L - 1 > 127) return refuse("landmark ids go through np.int8 (navigation_graph_safe.py:581)");
  if (cfg->adj_layout != LSM_ADJ_REFERENCE && cfg->adj_layout != LSM_ADJ_COMPACT)
    return refuse("adj_layout must be LSM_ADJ_REFERENCE or LSM_ADJ_COMPACT");
  if (cfg->scenario < LSM_SCENARIO_TRAIN || cfg->scenario > LSM_SCENARIO_DEPARTURES)
    return refuse("scenario must be LSM_SCENARIO_TRAIN, _LAYOUT or _DEPARTURES");
  if (cfg->rng != LSM_RNG_MT19937 && cfg->rng != LSM_RNG_PHILOX)
    return refuse("rng must be LSM_RNG_MT19937 or LSM_RNG_PHILOX");
  if (cfg->scenario != LSM_SCENARIO_TRAIN) {
    if (cfg->auto_reset)
      return refuse("layout scenarios are evaluation paths (GraphDummyVecEnv, scripts/eval_mpe.py): auto_reset must be 0");
    if (cfg->rng != LSM_RNG_MT19937) return refuse("layout scenarios draw on the host: rng must be LSM_RNG_MT19937");
  }
  if (cfg->scenario == LSM_SCENARIO_DEPARTURES && cfg->dynamics != LSM_AIRTAXI)
    return refuse("departure timers need airtaxi dynamics (RealisticScenario calls "
                  "reset_velocity(theta, speed), KinematicVehicleXYState only, core.py:137)");
  if (cfg->num_envs < 1) return refuse("num_envs must be >= 1");
  if (cfg->num_internal_step < 0 || cfg->num_internal_step > 64)
    return refuse("num_internal_step must be in [0, 64] (0 and 1: one inner step)");
  if (cfg->episode_length < 1) return refuse("episode_length must be >= 1");
  if (cfg->reward_terms & ~LSM_REWARD_ALL)
    return refuse("reward_terms: unknown LSM_REWARD_* bits (RewardBinaryConfig has four optional terms, "
                  "multiagent/config.py:78-83)");
  if (cfg->collaborative != 0 && cfg->collaborative != 1) return refuse("collaborative must be 0 or 1");
  const int dyn = cfg->dynamics == LSM_DOUBLE_INTEGRATOR ? 0 : 1;
  const bool nis1 = cfg->num_internal_step <= 1;
  k.rext = cfg->reward_terms != 0 || cfg->collaborative;
  k.block = N > MAXN || N * (1 + L) > MAXE || k.sel.workgroup_per_env == 1;
  // Lanes per env: 64 = one env per wave (default; measured fastest at 4096 envs, where
  // 4 waves/SIMD hide LDS/HBM latency), 32/16 = 2/4 envs per wave sharing the per-agent
  // instruction stream (needs N <= lanes). sel.lanes_per_env overrides.
  k.lpe = k.sel.lanes_per_env ? k.sel.lanes_per_env : 64;
  bool generic_only = k.sel.generic == 1;   // never use the compile-time-N kernels (tests)
  if (k.block) k.lpe = 64;   // lanes_per_env applies to the one-wave kernel only
  if (cfg->scenario != LSM_SCENARIO_TRAIN) {   // layouts: the generic one-wave kernel (mode 2 resets)
    generic_only = true;
    k.lpe = 64;
  }
  // the compile-time-N kernels are specialised on L = 2, the training setting; where the table has
  // no row for this N the family's generic kernel (NT = 0) runs
  const int nt = (L == 2 && !generic_only) ? N : 0;
  // Team kernel (lsm_team.h) for the compile-time-N BASELINE agent counts: G envs per
  // workgroup share one wave for their per-agent phases. sel.team = 0 selects rollout_kernel,
  // sel.team = G another instantiated G.
  k.team = 0;
  // the team kernel runs World.step's inner loop once (num_internal_step = 1, the training
  // default, train.sh:35); more inner steps run in rollout_kernel / the workgroup kernel
  if (!k.block && k.lpe == 64 && nt && nis1) {
    // default G = 4, measured (us/step): 4 < 8 < 2 (double integrator N = 8), lean LDS 4 < 2 < 0 (airtaxi N = 16)
    if (find_kernel(K_TEAM, dyn, nt, 4, true, k.rext)) k.team = 4;
    const int g = k.sel.team;
    if (g == 0) k.team = 0;
    else if (g > 0 && k.team && g * N <= 64) k.team = g;
    else if (g > 0 && k.team) return refuse("kernel select: team * num_agents must be <= 64");
  }
  // an explicit team size is honoured or refused: a parity test that asked for the team kernel
  // and got rollout_kernel would pass without running it
  if (k.sel.team > 0 && k.team != k.sel.team)
    return refuse("kernel select: team > 0 needs a team kernel instantiation (double integrator N = 8 or "
                  "airtaxi N = 16, 2 landmarks, lanes_per_env 64, num_internal_step <= 1, the training "
                  "scenario, neither generic nor workgroup_per_env)");
  // lean LDS layout for the airtaxi team kernel (6 -> 8 envs per CU at N = 16);
  // sel.lean = 0 keeps the full table (A/B)
  k.lean = k.team && cfg->dynamics == LSM_AIRTAXI && (N & 3) == 0 && ((N * (1 + L)) & 3) == 0;
  if (k.sel.lean == 0) k.lean = false;
  if (!(k.lpe == 16 || k.lpe == 32 || k.lpe == 64) || k.lpe < (k.block ? 1 : N))
    return refuse("kernel select: lanes_per_env must be 16, 32 or 64 and >= num_agents");
  if (k.team) {
    k.kernel = find_kernel(K_TEAM, dyn, nt, k.team, true, k.rext);
  } else {
    const int family = k.block ? K_BLOCK : K_WAVE, sub = k.block ? 0 : k.lpe;
    // the workgroup kernel that loops over inner steps always carries the optional-reward block
    const bool n1 = k.block && nis1, rx = k.block && (k.rext || !nis1);
    k.kernel = find_kernel(family, dyn, nt, sub, n1, rx);
    if (!k.kernel) k.kernel = find_kernel(family, dyn, 0, sub, n1, rx);
  }
  if (!k.kernel) return refuse("kernel select: no instantiated kernel for this configuration (lsm_kernels.h)");
  *out = k;
  return 0;
}

struct lsm_env {
  lsm_config cfg;
  int mt_stage = 2 * MT_N;   // KParams::mt_stage (lsm_test_set_mt_stage)
  uint16_t* pairs;
  int N, L, NL, E, F, OBS;
  StateDev s;
  std::vector<void*> allocs;
  void* out_ptr[LSM_NUM_OUT];
  size_t out_bytes[LSM_NUM_OUT];
  TableDev val, ttr;
  double ttr_max;
  double val_sep0;      // separation of the uploaded value table
  double sep_last;      // separation of the last reset / step call (chain-length bound)
  int sep_changes;      // changes of that separation since the table upload (>= any env's chain)
  std::string err;
  bool tables_ok;
  int device;
  KParams* dparams;   // device copy of the per-handle constants (re-uploaded when dirty)
  int32_t* action_err;   // device flag: an action index outside [0, 25) since the last check
  bool params_dirty;
  // ring-bound output slots (lsm_bind_output_ring): ring index i writes slot s at
  // ring_base[s] + (i + ring_off[s]) * ring_stride[s] when that lands in [0, ring_count[s]),
  // else at out_ptr[s]. One KParams copy per ring index lives in dring; selecting an index is a
  // host-side pointer choice (no upload, no sync per step).
  void* ring_base[LSM_NUM_OUT];
  size_t ring_stride[LSM_NUM_OUT];
  int32_t ring_count[LSM_NUM_OUT], ring_off[LSM_NUM_OUT];
  int32_t ring_len;    // number of ring indices (0: no ring slots)
  int32_t ring_cap;    // KParams copies allocated in dring
  int32_t ring_sel;    // -1: plain bindings
  KParams* dring;
  KernelChoice k;   // choose_kernel's answer for (cfg, lsm_create_select's select block)
};

static int fail(lsm_env* e, const std::string& msg) {
  if (e) e->err = msg;
  return 1;
}

// the reference builds an HjDataHandle (use_hj_handle, navigation_graph_safe.py:195)
static bool uses_hj(const lsm_env* e) {
  return e->cfg.use_safety_filter || (e->cfg.reward_terms & LSM_REWARD_HJ_VALUE);
}

#define HIPCHK(env, expr)                                                              \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess) return fail(env, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

template <class T>
static int dalloc(lsm_env* e, T** p, size_t count) {
  void* q = nullptr;
  hipError_t r = hipMalloc(&q, count * sizeof(T) + 16);
  if (r != hipSuccess) return fail(e, std::string("hipMalloc: ") + hipGetErrorString(r));
  e->allocs.push_back(q);
  *p = (T*)q;
  return 0;
}

static const KParams* active_params(const lsm_env* e) {
  return e->ring_sel >= 0 ? (const KParams*)(e->dring + e->ring_sel) : (const KParams*)e->dparams;
}

static void fill_params(const lsm_env* e, KParams& P) {
  memset(&P, 0, sizeof(P));
  const bool di = e->cfg.dynamics == LSM_DOUBLE_INTEGRATOR;
  P.n_envs = e->cfg.num_envs;
  P.N = e->N; P.L = e->L; P.NL = e->NL; P.E = e->E; P.F = e->F; P.OBS = e->OBS;
  P.dyn = di ? 0 : 1;
  P.episode_length = e->cfg.episode_length;
  P.use_masking = e->cfg.use_masking;
  P.use_filter_arg = e->cfg.use_safety_filter;
  P.auto_reset = e->cfg.auto_reset;
  P.adj_compact = e->cfg.adj_layout == LSM_ADJ_COMPACT;
  P.filter_search = e->k.sel.filter_search == 0 ? 0 : 1;
  P.scenario = e->cfg.scenario;
  P.rng = e->cfg.rng;
  P.nis = e->cfg.num_internal_step > 1 ? e->cfg.num_internal_step : 1;
  P.rbin = e->cfg.reward_terms;
  P.collab = e->cfg.collaborative ? 1 : 0;
  P.rext = e->k.rext ? 1 : 0;
  P.use_hj = (e->cfg.use_safety_filter || (e->cfg.reward_terms & LSM_REWARD_HJ_VALUE)) ? 1 : 0;
  P.mt_stage = e->mt_stage;
  P.seed = e->cfg.seed;
  P.env_offset = e->cfg.env_offset;
  P.lds_dep_off = (uint32_t)lds_plan(e->N, e->NL, e->E, e->F, e->k.block).bytes;
  P.lean = e->k.lean ? 1 : 0;
  P.world_size = e->cfg.world_size;
  const double pi = 3.141592653589793;
  P.pi = pi;
  P.two_pi = 2 * pi;
  if (di) {
    P.dt = 0.1; P.coord_range = 4; P.world_eng = 1.0; P.sep_target = 0.5;
    P.max_speed = 0.5; P.min_speed = 0.0; P.gs_min = 0.1; P.gs_max = 0.5;
    const double opts[5] = {-0.5, -0.25, 0.0, 0.25, 0.5};   // np.linspace(-0.5, 0.5, 5)
    for (int k = 0; k < 5; ++k) { P.act0[k] = opts[k]; P.act1[k] = opts[k]; }
  } else {
    P.dt = 1.0; P.coord_range = 3 * 1.60934; P.world_eng = 1.4; P.sep_target = 1500 * 0.0003048;
    P.max_speed = 175 * 0.514444 * 0.001; P.min_speed = 60 * 0.514444 * 0.001;
    P.gs_min = 60 * 0.514444 * 0.001; P.gs_max = 110 * 0.514444 * 0.001;
    // np.linspace(-0.1, 0.1, 5), np.linspace(-0.001, 0.002, 5)
    const double lo = -0.1, hi = 0.1, alo = -0.001, ahi = 0.002;
    for (int k = 0; k < 5; ++k) {
      P.act0[k] = (k == 4) ? hi : lo + k * ((hi - lo) / 4);
      P.act1[k] = (k == 4) ? ahi : alo + k * ((ahi - alo) / 4);
    }
  }
  {
    double t = P.coord_range * P.coord_range;
    while (std::sqrt(t) > P.coord_range) t = std::nextafter(t, 0.0);
    while (std::sqrt(std::nextafter(t, INFINITY)) <= P.coord_range) t = std::nextafter(t, INFINITY);
    P.coord_range_s = t;
  }
  {   // random_scenario_wave2's band, the device's products (lsm_team.h)
    const double dmin = di ? 0.25 * P.coord_range : 0.5 * P.coord_range;
    const double dmax = di ? 0.75 * P.coord_range : P.coord_range;
    double lo = dmin * dmin;
    while (std::sqrt(lo) > dmin) lo = std::nextafter(lo, 0.0);
    while (std::sqrt(std::nextafter(lo, INFINITY)) <= dmin) lo = std::nextafter(lo, INFINITY);
    double hi = dmax * dmax;
    while (std::sqrt(hi) < dmax) hi = std::nextafter(hi, INFINITY);
    while (std::sqrt(std::nextafter(hi, 0.0)) >= dmax) hi = std::nextafter(hi, 0.0);
    P.scen_d2lo = lo;
    P.scen_d2hi = hi;
  }
  P.cos_pi6 = cos(pi / 6);
  for (int k = 0; k < 50; ++k) {
    const double ph = k * ((2 * pi - 0) / 50);   // np.linspace(0, 2pi, 50, endpoint=False)
    P.mag_c[k] = cos(ph);
    P.mag_s[k] = sin(ph);
  }
  P.di_thr_xmax = 0.5 - 0.1 * 0.5; P.di_thr_xmin = -0.5 - 0.1 * -0.5;
  P.di_thr_ymax = 0.5 - 0.1 * 0.5; P.di_thr_ymin = -0.5 - 0.1 * -0.5;
  P.di_axmax = 0.5; P.di_axmin = -0.5; P.di_aymax = 0.5; P.di_aymin = -0.5;
  P.at_vmax = 175 * 0.514444 * 0.001; P.at_vmin = 60 * 0.514444 * 0.001;
  P.at_amax = 0.002; P.at_amin = -0.001; P.at_wmax = 0.1;
  P.at_thr_amax = P.at_vmax - 1.0 * 0.002; P.at_thr_amin = P.at_vmin - 1.0 * -0.001;
  P.at_box_w = (float)0.1; P.at_box_amax = (float)0.002; P.at_box_amin = (float)-0.001;
  auto magic = [](uint32_t d) { return (uint32_t)((((uint64_t)1 << 32) + d - 1) / d); };
  P.m_E = magic(e->E);
  P.m_EE = magic(e->E * e->E);
  P.m_EF = magic(e->E * e->F);
  P.m_F = magic(e->F);
  P.m_EF4 = magic(e->E * e->F / 4);
  P.m_NL = magic(e->NL);
  P.ttr_max = e->ttr_max;
  P.val_sep0 = e->val_sep0;
  P.val = e->val;
  P.ttr = e->ttr;
  P.s = e->s;
  P.o.obs = (float*)e->out_ptr[LSM_OUT_OBS];
  P.o.node = (float*)e->out_ptr[LSM_OUT_NODE_OBS];
  P.o.adj = (float*)e->out_ptr[LSM_OUT_ADJ];
  P.o.rew = (float*)e->out_ptr[LSM_OUT_REWARD];
  P.o.dones = (uint8_t*)e->out_ptr[LSM_OUT_DONE];
  P.o.reset_flag = (uint8_t*)e->out_ptr[LSM_OUT_RESET_FLAG];
  P.o.ep_info = (double*)e->out_ptr[LSM_OUT_EP_INFO];
  P.o.info = (double*)e->out_ptr[LSM_OUT_INFO];
  P.o.edges = (uint8_t*)e->out_ptr[LSM_OUT_EDGES];
  P.o.state = (double*)e->out_ptr[LSM_OUT_STATE];
  P.o.adjmask = (uint64_t*)e->out_ptr[LSM_OUT_ADJ_MASK];
  P.o.share_obs = (float*)e->out_ptr[LSM_OUT_SHARE_OBS];
  P.o.masks = (float*)e->out_ptr[LSM_OUT_MASKS];
  P.o.active_masks = (float*)e->out_ptr[LSM_OUT_ACTIVE_MASKS];
  P.o.cforce = e->cfg.collision_forces ? (double*)e->out_ptr[LSM_OUT_COLLISION_FORCE] : nullptr;
  P.o.departed = (uint8_t*)e->out_ptr[LSM_OUT_DEPARTED];
  P.o.adjnnz = (int64_t*)e->out_ptr[LSM_OUT_ADJ_NNZ];
  P.stamps = (unsigned long long*)e->out_ptr[LSM_OUT_DEBUG_STAMPS];
  P.diag = 0;
#ifdef LSM_STAMPS
  if (const char* v = getenv("LSM_DIAG")) P.diag = atoi(v);
#endif
  P.pairs = e->pairs;
  P.action_err = e->action_err;
}

extern "C" {

size_t lsm_output_bytes(const lsm_env* e, int32_t slot) {
  const size_t n = e->cfg.num_envs, N = e->N, E = e->E;
  switch (slot) {
    case LSM_OUT_OBS: return n * N * e->OBS * 4;
    case LSM_OUT_NODE_OBS: return n * N * E * e->F * 4;
    case LSM_OUT_ADJ: return (e->cfg.adj_layout == LSM_ADJ_COMPACT ? n : n * N) * E * E * 4;
    case LSM_OUT_ADJ_MASK: return n * N * ((E + 63) / 64) * 8;
    case LSM_OUT_REWARD: return n * N * 4;
    case LSM_OUT_DONE: return n * N;
    case LSM_OUT_RESET_FLAG: return n;
    case LSM_OUT_EP_INFO: return n * 8 * 8;
    case LSM_OUT_INFO: return n * N * LSM_INFO_FIELDS * 8;
    case LSM_OUT_EDGES: return n * E * E;
    case LSM_OUT_STATE: return n * N * 4 * 8;
    case LSM_OUT_DEBUG_STAMPS: return n * LSM_NSTAMP * 8;
    case LSM_OUT_SHARE_OBS: return n * N * N * e->OBS * 4;
    case LSM_OUT_MASKS: return n * N * 4;
    case LSM_OUT_ACTIVE_MASKS: return n * N * 4;
    case LSM_OUT_COLLISION_FORCE: return n * N * 2 * 8;
    case LSM_OUT_DEPARTED: return n * N;
    case LSM_OUT_ADJ_NNZ: return n * N * 8;
    default: return 0;
  }
}

int32_t lsm_num_entities(const lsm_env* e) { return e->E; }
int32_t lsm_layout_doubles(const lsm_env* e) {
  return e ? 4 * e->N + 4 * e->NL + (e->cfg.scenario == LSM_SCENARIO_DEPARTURES ? 3 * e->N : 0) + 1 : 0;
}
int32_t lsm_node_features(const lsm_env* e) { return e->F; }
int32_t lsm_obs_dim(const lsm_env* e) { return e->OBS; }
const char* lsm_last_error(const lsm_env* e) { return e ? e->err.c_str() : "null handle"; }

int lsm_create(const lsm_config* cfg, lsm_env** out) { return lsm_create_select(cfg, nullptr, out); }

int lsm_create_select(const lsm_config* cfg, const lsm_kernel_select* sel, lsm_env** out) {
  *out = nullptr;
  if (!cfg) return 1;
  lsm_env* e = new lsm_env();
  *out = e;
  e->cfg = *cfg;
  e->tables_ok = false;
  e->dparams = nullptr;
  for (int k = 0; k < LSM_NUM_OUT; ++k) {
    e->ring_base[k] = nullptr; e->ring_stride[k] = 0; e->ring_count[k] = 0; e->ring_off[k] = 0;
  }
  e->ring_len = 0; e->ring_cap = 0; e->ring_sel = -1; e->dring = nullptr;
  e->params_dirty = true;
  e->ttr_max = 0.0;
  e->val_sep0 = e->sep_last = 0.0;
  e->sep_changes = 0;
  memset(&e->val, 0, sizeof(e->val));
  memset(&e->ttr, 0, sizeof(e->ttr));
  for (int k = 0; k < LSM_NUM_OUT; ++k) { e->out_ptr[k] = nullptr; e->out_bytes[k] = 0; }
  if (choose_kernel(cfg, sel, &e->k, &e->err)) return 1;
  const int N = cfg->num_agents, L = cfg->num_landmarks;
  e->N = N; e->L = L; e->NL = N * L; e->E = N * (1 + L);
  e->F = cfg->dynamics == LSM_DOUBLE_INTEGRATOR ? 10 : 11;
  e->OBS = cfg->dynamics == LSM_DOUBLE_INTEGRATOR ? 7 : 6;
  HIPCHK(e, hipGetDevice(&e->device));
  const size_t n = cfg->num_envs;
  int r = 0;
  const LdsPlan lp = lds_plan(N, e->NL, e->E, e->F, e->k.block);
  e->s.rec16 = (uint32_t)(lp.rec / 16);
  e->s.a1_16 = (uint32_t)(lp.a1 / 16);
  e->s.a2_16 = (uint32_t)(lp.a2 / 16);
  e->s.a3_16 = (uint32_t)(lp.a3 / 16);
  e->s.rec_stride16 = (uint32_t)(((lp.rec + 127) / 128) * 8);   // 128-B aligned records
  r |= dalloc(e, &e->s.rec, n * e->s.rec_stride16);
  r |= dalloc(e, &e->s.prev, n * 8);
  r |= dalloc(e, &e->dparams, 1);
  r |= dalloc(e, &e->s.mt, n * MT_WORDS);
  r |= dalloc(e, &e->pairs, (size_t)e->E * (e->E - 1) / 2 + 1);
  r |= dalloc(e, &e->action_err, 1);
  e->s.dep = nullptr;
  e->s.sepx = nullptr;
  e->s.sepx_cap = 0;
  if (cfg->scenario == LSM_SCENARIO_DEPARTURES) r |= dalloc(e, &e->s.dep, n * depw(N));
  if (r) return 1;
  if (e->s.dep) {   // Agent.departed defaults to True (core.py:343), timers 0
    std::vector<double> d(n * depw(N), 0.0);
    for (size_t k = 0; k < n; ++k)
      for (int i = 0; i < N; ++i) d[k * depw(N) + i] = 1.0;
    HIPCHK(e, hipMemcpy(e->s.dep, d.data(), d.size() * 8, hipMemcpyHostToDevice));
  }
  HIPCHK(e, hipMemset(e->action_err, 0, sizeof(int32_t)));
  {
    // agent-agent pairs first (the only ones needing the float64 blocks), then
    // agent-landmark, then landmark-landmark: the agent block stays in the first lane pass
    std::vector<uint16_t> pr;
    for (int cls = 0; cls < 3; ++cls)
      for (int a = 0; a < e->E; ++a)
        for (int b = a + 1; b < e->E; ++b) {
          const int c = (a < N ? 0 : 1) + (b < N ? 0 : 1);
          if (c == cls) pr.push_back((uint16_t)(a | (b << 8)));
        }
    pr.push_back(0);
    HIPCHK(e, hipMemcpy(e->pairs, pr.data(), pr.size() * 2, hipMemcpyHostToDevice));
  }
  {
    // reference initial values: prev summary (environment.py:873-881), stats and info
    // accumulators (init_episode_agent_info), decon -1, min distances inf
    const size_t stride = (size_t)e->s.rec_stride16 * 16;
    std::vector<unsigned char> rec(stride, 0);
    double* stats = (double*)(rec.data() + lp.off[REC_STATS]);
    double* winfo = (double*)(rec.data() + lp.off[REC_WINFO]);
    double* gmt = (double*)(rec.data() + lp.off[REC_GMT]);
    double* minrel = (double*)(rec.data() + lp.off[REC_MINREL]);
    int32_t* decon = (int32_t*)(rec.data() + lp.off[REC_DECON]);
    for (int i = 0; i < N; ++i) {
      stats[4 * N + i] = INFINITY;
      for (int q = 0; q < 3; ++q) winfo[q * N + i] = -1.0;
      winfo[3 * N + i] = 0.0;
      gmt[i] = INFINITY;
      minrel[i] = INFINITY;
      decon[i] = -1;
    }
    std::vector<unsigned char> all(n * stride);
    for (size_t k = 0; k < n; ++k) memcpy(all.data() + k * stride, rec.data(), stride);
    HIPCHK(e, hipMemcpy(e->s.rec, all.data(), all.size(), hipMemcpyHostToDevice));
    std::vector<double> prev(n * 8, 0.0);
    for (size_t k = 0; k < n; ++k) prev[k * 8 + 0] = cfg->episode_length;
    HIPCHK(e, hipMemcpy(e->s.prev, prev.data(), prev.size() * 8, hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(seed_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, e->s.mt, (int)n, cfg->seed,
                     cfg->env_offset);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipDeviceSynchronize());
  e->tables_ok = !uses_hj(e) && cfg->dynamics == LSM_DOUBLE_INTEGRATOR;
  return 0;
}

void lsm_destroy(lsm_env* e) {
  if (!e) return;
  for (void* p : e->allocs) (void)hipFree(p);
  delete e;
}

// Free one of the handle's allocations (a replaced table).
static void dfree(lsm_env* e, const void* p) {
  if (!p) return;
  for (size_t k = 0; k < e->allocs.size(); ++k)
    if (e->allocs[k] == p) {
      (void)hipFree(e->allocs[k]);
      e->allocs.erase(e->allocs.begin() + k);
      return;
    }
}

static int upload_table(lsm_env* e, TableDev& T, int32_t ndim, const double* lo, const double* hi,
                        const int32_t* shape, const int32_t* periodic, const float* values,
                        const float* grads) {
  if (ndim < 1 || ndim > 5) return fail(e, "table ndim must be in [1, 5]");
  HIPCHK(e, hipDeviceSynchronize());   // a replaced table may still be read by queued launches
  dfree(e, T.cells);
  dfree(e, T.gcells);
  dfree(e, T.bnd);
  memset(&T, 0, sizeof(T));
  T.ndim = ndim;
  size_t nodes = 1, cells = 1;
  for (int d = 0; d < ndim; ++d) {
    if (shape[d] < 2) return fail(e, "table dims must have >= 2 nodes");
    nodes *= (size_t)shape[d];
    cells *= (size_t)(periodic[d] ? shape[d] : shape[d] - 1);
  }
  size_t cst = 1;
  for (int d = ndim - 1; d >= 0; --d) {
    T.n[d] = shape[d];
    T.cstride[d] = (int)cst;
    cst *= (size_t)(periodic[d] ? shape[d] : shape[d] - 1);
    T.periodic[d] = periodic[d] ? 1 : 0;
    const double sp = T.periodic[d] ? (hi[d] - lo[d]) / shape[d] : (hi[d] - lo[d]) / (shape[d] - 1.0);
    T.lo[d] = (float)lo[d];
    T.sp[d] = (float)sp;
  }
  // grid_pos's reciprocal path, per dimension, where it equals the division for every y = s - lo
  // a lookup can meet: grid positions within [-4, n + 3] (non-periodic: outside, the lookup is out
  // of the grid either way -- a faithful quotient cannot cross those bounds) or within 1e9 in
  // magnitude (periodic: the wrap reads the position itself; beyond 1e9 grid_cell refuses it)
  {
    int* bad = nullptr;
    HIPCHK(e, hipMalloc((void**)&bad, sizeof(int)));
#ifdef LSM_DIAGNOSTIC_BUILD
    const bool no_mdiv = getenv("LSM_NO_MDIV") != nullptr;   // A/B of the division path (variant builds)
#else
    const bool no_mdiv = false;   // the product reads no environment knobs
#endif
    for (int d = 0; d < ndim; ++d) {
      T.rsp[d] = 1.0f / T.sp[d];
      T.mdiv[d] = 0;
      if (!(T.sp[d] > 0.0f) || no_mdiv) continue;
      const float plo = T.periodic[d] ? -1.0e9f : -4.0f;
      const float phi = T.periodic[d] ? 1.0e9f : (float)(T.n[d] + 3);
      const float ypos = phi * T.sp[d] * 1.0001f, yneg = -plo * T.sp[d] * 1.0001f;
      uint32_t pb, nb;
      memcpy(&pb, &ypos, 4);
      memcpy(&nb, &yneg, 4);
      HIPCHK(e, hipMemset(bad, 0, sizeof(int)));
      hipLaunchKernelGGL(mdiv_check_kernel, dim3(4096), dim3(256), 0, 0, T.sp[d], T.rsp[d], pb, nb, bad);
      HIPCHK(e, hipGetLastError());
      int h = 1;
      HIPCHK(e, hipMemcpy(&h, bad, sizeof(int), hipMemcpyDeviceToHost));
      T.mdiv[d] = h == 0 ? 1 : 0;
    }
    HIPCHK(e, hipFree(bad));
  }
  const size_t ncorner = (size_t)1 << ndim;
  if (cells * ncorner * 2 > (size_t)INT32_MAX) return fail(e, "table too large for 32-bit cell offsets");
  T.gw = ndim <= 4 ? 1 : 2;
  float* dv = nullptr;
  float4* dg = nullptr;
  HIPCHK(e, hipMalloc((void**)&dv, nodes * 4));
  HIPCHK(e, hipMemcpy(dv, values, nodes * 4, hipMemcpyHostToDevice));
  if (grads) {
    HIPCHK(e, hipMalloc((void**)&dg, nodes * T.gw * 16));
    HIPCHK(e, hipMemcpy(dg, grads, nodes * T.gw * 16, hipMemcpyHostToDevice));
  }
  float* cv = nullptr;
  float4* cg = nullptr;
  if (dalloc(e, &cv, cells * ncorner)) return 1;
  if (grads && dalloc(e, &cg, cells * ncorner * T.gw)) return 1;
  const int64_t work = (int64_t)(cells * ncorner);
  hipLaunchKernelGGL(expand_cells_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, 0, dv, dg, cv, cg,
                     T, (int64_t)cells);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipDeviceSynchronize());
  HIPCHK(e, hipFree(dv));
  if (dg) HIPCHK(e, hipFree(dg));
  T.cells = cv;
  T.gcells = cg;
  return 0;
}

// Value bounds per 4^ndim-cell block (TableDev::bnd), built from the node table.
static int upload_bounds(lsm_env* e, TableDev& T, const float* values) {
  // 4 cells per dim: 180 KB for the full DI table (L2-resident); sel.bounds_shift for tests
  T.bshift = e->k.sel.bounds_shift ? e->k.sel.bounds_shift : 2;
  const int B = 1 << T.bshift;
  int nblocks = 1;
  for (int d = T.ndim - 1; d >= 0; --d) {
    const int ncell = T.periodic[d] ? T.n[d] : T.n[d] - 1;
    T.bstride[d] = nblocks;
    nblocks *= (ncell + B - 1) / B;
  }
  size_t nodes = 1;
  for (int d = 0; d < T.ndim; ++d) nodes *= (size_t)T.n[d];
  float* dv = nullptr;
  HIPCHK(e, hipMalloc((void**)&dv, nodes * 4));
  HIPCHK(e, hipMemcpy(dv, values, nodes * 4, hipMemcpyHostToDevice));
  float2* bd = nullptr;
  if (dalloc(e, &bd, (size_t)nblocks)) return 1;
  hipLaunchKernelGGL(bounds_kernel, dim3((nblocks + 255) / 256), dim3(256), 0, 0, dv, bd, T, nblocks);
  HIPCHK(e, hipGetLastError());
  HIPCHK(e, hipDeviceSynchronize());
  HIPCHK(e, hipFree(dv));
  T.bnd = bd;
  return 0;
}

int lsm_set_value_table(lsm_env* e, int32_t ndim, const double* lo, const double* hi, const int32_t* shape,
                        const int32_t* periodic, const float* values, const float* grads,
                        double separation_distance) {
  const int want = e->cfg.dynamics == LSM_DOUBLE_INTEGRATOR ? 4 : 5;
  if (ndim != want) return fail(e, "value table must be 4-D (double integrator) or 5-D (airtaxi)");
  if (!grads) return fail(e, "value table needs its gradient table");
  if (upload_table(e, e->val, ndim, lo, hi, shape, periodic, values, grads)) return 1;
  if (upload_bounds(e, e->val, values)) return 1;
  e->val_sep0 = e->sep_last = separation_distance;
  e->sep_changes = 0;
  {
    const LdsPlan lp = lds_plan(e->N, e->NL, e->E, e->F, e->k.block);
    const int n = e->cfg.num_envs;
    hipLaunchKernelGGL(sep_clear_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, e->s.rec, e->s.rec_stride16, n,
                       (uint32_t)(lp.off[REC_CUR] + 8 * NCUR));
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipDeviceSynchronize());
  }
  e->tables_ok = (e->cfg.dynamics == LSM_DOUBLE_INTEGRATOR) || e->ttr.cells != nullptr;
  e->params_dirty = true;
  return 0;
}

int lsm_set_ttr_table(lsm_env* e, int32_t ndim, const double* lo, const double* hi, const int32_t* shape,
                      const int32_t* periodic, const float* values, double ttr_max) {
  if (ndim != 4) return fail(e, "TTR table must be 4-D");
  if (upload_table(e, e->ttr, ndim, lo, hi, shape, periodic, values, nullptr)) return 1;
  e->ttr_max = ttr_max;
  e->tables_ok = !uses_hj(e) || e->val.cells != nullptr;
  e->params_dirty = true;
  return 0;
}

int lsm_bind_output(lsm_env* e, int32_t slot, void* ptr, size_t bytes) {
  if (slot < 0 || slot >= LSM_NUM_OUT) return fail(e, "bad output slot");
  const size_t need = lsm_output_bytes(e, slot);
  if (ptr && bytes < need) return fail(e, "output buffer too small for slot " + std::to_string(slot));
  e->out_ptr[slot] = ptr;
  e->params_dirty = true;
  e->out_bytes[slot] = bytes;
  return 0;
}

int lsm_bind_output_ring(lsm_env* e, int32_t slot, void* base, size_t stride_bytes, int32_t count,
                         int32_t index_offset) {
  if (!e) return 1;
  if (slot < 0 || slot >= LSM_NUM_OUT) return fail(e, "bad output slot");
  if (slot == LSM_OUT_RESET_FLAG || slot == LSM_OUT_EP_INFO || slot == LSM_OUT_EDGES ||
      slot == LSM_OUT_DEBUG_STAMPS || slot == LSM_OUT_DEPARTED || slot == LSM_OUT_ADJ_NNZ)
    return fail(e, "slot " + std::to_string(slot) + " cannot be ring-bound");
  if (count <= 0 || !base) {   // unbind
    e->ring_count[slot] = 0;
  } else {
    if (stride_bytes < lsm_output_bytes(e, slot))
      return fail(e, "ring stride smaller than slot " + std::to_string(slot) + "'s output");
    e->ring_base[slot] = base;
    e->ring_stride[slot] = stride_bytes;
    e->ring_count[slot] = count;
    e->ring_off[slot] = index_offset;
  }
  int len = 0;
  for (int s = 0; s < LSM_NUM_OUT; ++s)
    if (e->ring_count[s] > 0) len = std::max(len, e->ring_count[s] - e->ring_off[s]);
  e->ring_len = len;
  if (e->ring_sel >= len) e->ring_sel = -1;
  e->params_dirty = true;
  return 0;
}

int lsm_select_ring(lsm_env* e, int32_t index) {
  if (!e) return 1;
  if (index < -1 || index >= e->ring_len)
    return fail(e, "ring index " + std::to_string(index) + " outside [-1, " + std::to_string(e->ring_len) + ")");
  e->ring_sel = index;
  return 0;
}

static int check_ready(lsm_env* e, bool stepping) {
  if (!e->tables_ok) return fail(e, "HJ value table (filter on) / TTR table (airtaxi) not set");
  const int req[] = {LSM_OUT_OBS, LSM_OUT_NODE_OBS, LSM_OUT_ADJ, LSM_OUT_REWARD, LSM_OUT_DONE,
                     LSM_OUT_RESET_FLAG, LSM_OUT_EP_INFO, LSM_OUT_INFO};
  for (int s : req)
    if (!e->out_ptr[s]) return fail(e, "output slot " + std::to_string(s) + " not bound");
  if (e->cfg.adj_layout == LSM_ADJ_COMPACT && !e->out_ptr[LSM_OUT_ADJ_MASK])
    return fail(e, "compact adjacency layout needs LSM_OUT_ADJ_MASK bound");
  if (e->cfg.collision_forces && !e->out_ptr[LSM_OUT_COLLISION_FORCE])
    return fail(e, "collision_forces needs LSM_OUT_COLLISION_FORCE bound");
  if (e->k.block && e->out_ptr[LSM_OUT_ADJ_NNZ])
    return fail(e, "LSM_OUT_ADJ_NNZ is written by the one-wave and team kernels (E <= 64); the workgroup-per-env "
                   "kernel's edge lists take lsm_edges_count's pass");
  (void)stepping;
  return 0;
}

// An env's shift chain grows only at its resets, by one entry per change of the separation it
// resets with, so the changes across the calls' curriculum blocks since the table upload bound every
// chain. The record holds KSEP shifts; before a launch that could write shift k >= KSEP the per-env
// overflow rows (StateDev::sepx) are grown, stream-ordered, keeping the shifts already there. The
// reference has no bound (HjDataHandle.update_separation_distance shifts the table in place,
// safety_filter.py:170-174); neither has this.
static int sep_check(lsm_env* e, const lsm_curriculum* cur, hipStream_t st) {
  if (!uses_hj(e)) return 0;
  if (cur->separation_distance == e->sep_last) return 0;
  // the overflow rows are grown first; the change is recorded only once they can hold it, so a
  // failed allocation leaves the handle as it was (a retry grows them again)
  const int changes = e->sep_changes + 1;
  const uint32_t need = changes > KSEP ? (uint32_t)(changes - KSEP) : 0;
  if (need > e->s.sepx_cap) {
    const uint32_t cap = std::max<uint32_t>(std::max<uint32_t>(2 * e->s.sepx_cap, 16), need);
    const size_t n = (size_t)e->cfg.num_envs;
    double* nx = nullptr;
    if (dalloc(e, &nx, n * cap)) return 1;
    if (e->s.sepx) {
      if (hipMemcpy2DAsync(nx, (size_t)cap * 8, e->s.sepx, (size_t)e->s.sepx_cap * 8, (size_t)e->s.sepx_cap * 8, n,
                           hipMemcpyDeviceToDevice, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess) {
        dfree(e, nx);
        return fail(e, "growing the HJ separation shift rows failed");
      }
      dfree(e, e->s.sepx);
    }
    e->s.sepx = nx;
    e->s.sepx_cap = cap;
    e->params_dirty = true;
  }
  e->sep_changes = changes;
  e->sep_last = cur->separation_distance;
  return 0;
}

// output pointers of ring index i (see lsm_env::ring_*)
static void apply_ring(const lsm_env* e, int i, KParams& P) {
  auto at = [&](int slot, void* plain) -> void* {
    if (e->ring_count[slot] <= 0) return plain;
    const int j = i + e->ring_off[slot];
    if (j < 0 || j >= e->ring_count[slot]) return plain;
    return (char*)e->ring_base[slot] + (size_t)j * e->ring_stride[slot];
  };
  P.o.obs = (float*)at(LSM_OUT_OBS, P.o.obs);
  P.o.node = (float*)at(LSM_OUT_NODE_OBS, P.o.node);
  P.o.adj = (float*)at(LSM_OUT_ADJ, P.o.adj);
  P.o.rew = (float*)at(LSM_OUT_REWARD, P.o.rew);
  P.o.dones = (uint8_t*)at(LSM_OUT_DONE, P.o.dones);
  P.o.info = (double*)at(LSM_OUT_INFO, P.o.info);
  P.o.state = (double*)at(LSM_OUT_STATE, P.o.state);
  P.o.adjmask = (uint64_t*)at(LSM_OUT_ADJ_MASK, P.o.adjmask);
  P.o.share_obs = (float*)at(LSM_OUT_SHARE_OBS, P.o.share_obs);
  P.o.masks = (float*)at(LSM_OUT_MASKS, P.o.masks);
  P.o.active_masks = (float*)at(LSM_OUT_ACTIVE_MASKS, P.o.active_masks);
  P.o.cforce = (double*)at(LSM_OUT_COLLISION_FORCE, P.o.cforce);
}

static int launch(lsm_env* e, KStep& L, hipStream_t st) {
  size_t env_lds = lds_plan(e->N, e->NL, e->E, e->F, e->k.block, e->k.lean).bytes;
  if (e->k.team) env_lds = team_env_bytes(env_lds, e->N);
  if (e->cfg.scenario == LSM_SCENARIO_DEPARTURES) env_lds += dep_lds_bytes(e->N);
  if (e->k.block ? env_lds > 160 * 1024
                 : (e->k.team ? env_lds * e->k.team > 160 * 1024 : env_lds * (WAVE / e->k.lpe) > 65536))
    return fail(e, "LDS footprint too large");
  if (e->params_dirty) {   // outputs / tables changed: refresh the device copy (stream-ordered)
    KParams P;
    fill_params(e, P);
    P.lds_env_bytes = (uint32_t)env_lds;
    HIPCHK(e, hipMemcpyAsync(e->dparams, &P, sizeof(P), hipMemcpyHostToDevice, st));
    if (e->ring_len > 0) {
      if (e->ring_cap < e->ring_len) {
        if (dalloc(e, &e->dring, (size_t)e->ring_len)) return 1;
        e->ring_cap = e->ring_len;
      }
      std::vector<KParams> ring((size_t)e->ring_len);
      for (int i = 0; i < e->ring_len; ++i) {
        ring[i] = P;
        apply_ring(e, i, ring[i]);
      }
      HIPCHK(e, hipMemcpyAsync(e->dring, ring.data(), sizeof(KParams) * ring.size(), hipMemcpyHostToDevice, st));
    }
    HIPCHK(e, hipStreamSynchronize(st));
    e->params_dirty = false;
  }
  L.stop_after = -1;
#ifdef LSM_STAMPS
  if (const char* v = getenv("LSM_STOP_AFTER")) L.stop_after = atoi(v);
#endif
  if (const int rc = e->k.kernel->launch(active_params(e), e->cfg.num_envs, L, env_lds, st))
    return fail(e, std::string(e->k.kernel->name) + ": hipFuncSetAttribute(MaxDynamicSharedMemorySize): " +
                       hipGetErrorString((hipError_t)rc));
  HIPCHK(e, hipGetLastError());
  return 0;
}

#ifndef LSM_BUILD_ID
#define LSM_BUILD_ID "unknown"
#endif
const char* lsm_build_id(void) { return LSM_BUILD_ID; }

int lsm_test_set_mt_stage(lsm_env* e, int32_t words) {
  if (!e) return 1;
  e->mt_stage = std::max(1, std::min(2 * MT_N, (int)words));
  e->params_dirty = true;
  return 0;
}

int lsm_test_read_value_bounds(lsm_env* e, float* lo_hi, int32_t cap_blocks, int32_t nblocks_per_dim[5],
                               int32_t* bshift) {
  if (!e) return 1;
  const TableDev& T = e->val;
  if (!T.bnd || T.ndim < 1) return fail(e, "read value bounds: no value table set");
  if (!lo_hi || !nblocks_per_dim || !bshift) return fail(e, "read value bounds: null argument");
  const int B = 1 << T.bshift;
  int64_t nblocks = 1;
  for (int d = 0; d < 5; ++d) {
    nblocks_per_dim[d] = 0;
    if (d >= T.ndim) continue;
    const int ncell = T.periodic[d] ? T.n[d] : T.n[d] - 1;
    nblocks_per_dim[d] = (ncell + B - 1) / B;
    nblocks *= nblocks_per_dim[d];
  }
  *bshift = T.bshift;
  if ((int64_t)cap_blocks < nblocks) return fail(e, "read value bounds: capacity below the table's block count");
  HIPCHK(e, hipDeviceSynchronize());
  HIPCHK(e, hipMemcpy(lo_hi, T.bnd, (size_t)nblocks * sizeof(float2), hipMemcpyDeviceToHost));
  return 0;
}

// The kernel launch() runs for this handle: the chosen row of the kernel table.
const char* lsm_kernel_name(const lsm_env* e) { return e && e->k.kernel ? e->k.kernel->name : ""; }

int lsm_kernel_name_for(const lsm_config* cfg, const lsm_kernel_select* sel, char* buf, size_t cap) {
  if (!cfg || !buf || cap == 0) return 1;
  KernelChoice k;
  std::string text;
  int rc = choose_kernel(cfg, sel, &k, &text);
  if (!rc) text = k.kernel->name;
  if (text.size() >= cap) rc = 1;   // truncated: not an answer
  snprintf(buf, cap, "%s", text.c_str());
  return rc;
}

int lsm_set_agent_state(lsm_env* e, int32_t env_index, const double* state, const int32_t* reached,
                        void* stream) {
  if (!e || !state) return 1;
  if (env_index < 0 || env_index >= e->cfg.num_envs) return fail(e, "env_index out of range");
  HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
  const LdsPlan lp = lds_plan(e->N, e->NL, e->E, e->F, e->k.block);
  std::vector<unsigned char> rec(lp.rec);
  float4* dev = e->s.rec + (size_t)env_index * e->s.rec_stride16;
  HIPCHK(e, hipMemcpy(rec.data(), dev, lp.rec, hipMemcpyDeviceToHost));
  double* ps = (double*)(rec.data() + lp.off[REC_PS]);   // agent state [4][N]
  for (int i = 0; i < e->N; ++i)
    for (int c = 0; c < 4; ++c) ps[c * e->N + i] = state[i * 4 + c];
  if (reached) {
    int32_t* rp = (int32_t*)(rec.data() + lp.off[REC_REACHED]);
    for (int i = 0; i < e->N; ++i) rp[i] = reached[i];
  }
  ((int32_t*)(rec.data() + lp.off[REC_STEP]))[1] = 1;   // step slot: distances recomputed, unmasked
  HIPCHK(e, hipMemcpy(dev, rec.data(), lp.rec, hipMemcpyHostToDevice));
  return 0;
}

int lsm_reset(lsm_env* e, const lsm_curriculum* cur, void* stream) {
  if (!e || !cur) return 1;
  if (e->cfg.scenario != LSM_SCENARIO_TRAIN) return fail(e, "layout scenario: reset with lsm_reset_layout");
  if (check_ready(e, false)) return 1;
  if (sep_check(e, cur, (hipStream_t)stream)) return 1;
  KStep L;
  memset(&L, 0, sizeof(L));
  memcpy(L.cur_new, cur, sizeof(double) * NCUR);
  L.mode = 1;
  L.emit_edges = 0;
  return launch(e, L, (hipStream_t)stream);
}

int lsm_reset_layout(lsm_env* e, const lsm_curriculum* cur, const double* layout, void* stream) {
  if (!e || !cur) return 1;
  if (e->cfg.scenario == LSM_SCENARIO_TRAIN) return fail(e, "lsm_reset_layout needs a layout scenario");
  if (!layout) return fail(e, "null layout");
  if (check_ready(e, false)) return 1;
  if (sep_check(e, cur, (hipStream_t)stream)) return 1;
  KStep L;
  memset(&L, 0, sizeof(L));
  memcpy(L.cur_new, cur, sizeof(double) * NCUR);
  L.mode = 2;
  L.layout = layout;
  return launch(e, L, (hipStream_t)stream);
}

int lsm_step(lsm_env* e, const void* actions, int32_t kind, const lsm_curriculum* cur, void* stream) {
  if (!e || !actions || !cur) return fail(e, "null argument");
  if (kind < 0 || kind > 2) return fail(e, "bad action kind");
  if (check_ready(e, true)) return 1;
  // a step's curriculum block is used only by its auto-resets: without them no chain can grow
  if (e->cfg.auto_reset && sep_check(e, cur, (hipStream_t)stream)) return 1;
  KStep L;
  memset(&L, 0, sizeof(L));
  memcpy(L.cur_new, cur, sizeof(double) * NCUR);
  L.mode = 0;
  L.action_kind = kind;
  L.actions = actions;
  L.emit_edges = e->cfg.emit_edges && e->out_ptr[LSM_OUT_EDGES] != nullptr;
  return launch(e, L, (hipStream_t)stream);
}

int32_t lsm_action_errors(lsm_env* e, void* stream) {
  if (!e) return -1;
  int32_t v = 0;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
  if (hipMemcpy(&v, e->action_err, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (v && hipMemset(e->action_err, 0, sizeof(int32_t)) != hipSuccess) return -1;
  return v;
}

int lsm_host_rk45_di(const double* y0, double a0, double a1, double dt, double* y_out) {
  double y[4] = {y0[0], y0[1], y0[2], y0[3]};
  const int n = rk45_di(y, a0, a1, dt);
  for (int i = 0; i < 4; ++i) y_out[i] = y[i];
  return n;
}

double lsm_host_glibc_pow(double x, double y) { return glibc_pow(x, y); }

int lsm_host_philox4x32(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  philox4x32_10(ctr, key, out);
  return 0;
}

int lsm_host_philox_uniforms(uint32_t key, uint32_t reset_index, int32_t count, double lo, double hi,
                             double* out) {
  Philox m;
  m.init(key, reset_index);
  for (int k = 0; k < count; ++k) out[k] = m.uniform(lo, hi);
  return 0;
}

int lsm_host_mt_uniforms(uint32_t seed, int32_t count, double lo, double hi, double* out) {
  HostMT m;
  m.seed(seed);
  for (int k = 0; k < count; ++k) out[k] = m.uniform(lo, hi);
  return 0;
}

int lsm_host_scenario(const lsm_config* cfg, const lsm_curriculum* cur, uint32_t seed, double* agent_state,
                      double* landmarks) {
  const int N = cfg->num_agents, L = cfg->num_landmarks, NL = N * L;
  if (N < 2 || N > BMAXN || L < 2 || L > MAX_L) return 1;
  ScenarioParams sp;
  const bool di = cfg->dynamics == LSM_DOUBLE_INTEGRATOR;
  sp.dyn = di ? 0 : 1; sp.N = N; sp.L = L; sp.world_size = cfg->world_size;
  sp.coordination_range = di ? 4.0 : 3 * 1.60934;
  sp.goal_speed_min = di ? 0.1 : 60 * 0.514444 * 0.001;
  sp.goal_speed_max = di ? 0.5 : 110 * 0.514444 * 0.001;
  sp.ratio_airtaxi = cur->ratio_airtaxi; sp.ratio_scenario = cur->ratio_scenario;
  sp.pi = 3.141592653589793; sp.two_pi = 2 * sp.pi;
  sp.d2lo = sp.d2hi = 0.0;   // (the device draw's squared band; random_scenario tests d itself)
  std::vector<double> st(4 * N), lm(4 * NL), ws(SCEN_WS);
  if (cfg->rng == LSM_RNG_PHILOX) {   // the device's first reset (reset index 0) of this seed
    Philox m;
    m.init(seed, 0);
    random_scenario(m, sp, st.data(), lm.data(), ws.data());
  } else {
    HostMT m;
    m.seed(seed);
    random_scenario(m, sp, st.data(), lm.data(), ws.data());
  }
  for (int i = 0; i < N; ++i)
    for (int c = 0; c < 4; ++c) agent_state[i * 4 + c] = st[c * N + i];
  for (int k = 0; k < NL; ++k)
    for (int c = 0; c < 4; ++c) landmarks[k * 4 + c] = lm[c * NL + k];
  return 0;
}

}  // extern "C"

