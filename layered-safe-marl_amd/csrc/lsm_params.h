// lsm_params.h -- what the step kernels (lsm_rollout.hip) and the host side of the C ABI
// (lsm_host.hip) share: the limits, the device-resident parameter block of a handle (KParams) and
// the per-launch arguments (KStep), the LDS / record layout (lds_plan) and the few helpers both
// sides evaluate. It also holds the product build's guard against diagnostic switches, so that
// guard protects every translation unit of the rollout.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/lsm_rollout.h"
#include "lsm_numeric.h"
#include "lsm_scenario.h"

// Diagnostic switches (bounds that compute wrong results on purpose, in-kernel stamps) exist only in
// variant builds (lsm.build.build_variants defines LSM_DIAGNOSTIC_BUILD); the product refuses them.
#if !defined(LSM_DIAGNOSTIC_BUILD) &&                                                              \
    (defined(LSM_STAMPS) || defined(LSM_XP_VALHOT) || defined(LSM_XP_GRADHOT) || defined(LSM_XP_NOFILT) || \
     defined(LSM_XP_NOOUT) || defined(LSM_XP_NORESETEMIT) || defined(LSM_XP_NORK) || defined(LSM_XP_NOSCEN) || \
     defined(LSM_XP_DELAY) || defined(LSM_XP_POISON))
#error "diagnostic switch in a product build: use lsm.build.build_variants (LSM_DIAGNOSTIC_BUILD)"
#endif

// stamps per env in LSM_OUT_DEBUG_STAMPS: 16 in the ABI; diagnostic builds stamp 40
#ifdef LSM_STAMPS
#define LSM_NSTAMP 40
#else
#define LSM_NSTAMP 16
#endif

namespace lsm {

constexpr int WAVE = 64;
constexpr int MAXN = 32;        // agents per env supported by the one-wave kernel
constexpr int MAXE = 64;        // entities per env (N * (1 + L))
constexpr int MT_WORDS = MT_N + 1;  // key[624] + pos
constexpr int NCUR = 12;
constexpr int NSTAT = 6;        // travel_length, travel_distance, done, conflict, min_distance, multiple
constexpr int NWINFO = 4;       // times_required, dists_to_goal, dist_left_to_goal, num_agent_collisions
// Per-env HJ separation history (record, after cur): HjDataHandle.update_separation_distance
// (safety_filter.py:170-174) runs `values_hj -= shift` on every reset of every env, so each env's
// table is the uploaded one minus its own chain of float64 shifts, each rounded to float32
// (numpy: float32 array -= float64 scalar). sep[0] = number of shifts, sep[1] = the env's current
// separation (sep[0] == 0: the uploaded table's, KParams::val_sep0), sep[2 + k] = shift k for
// k < KSEP; longer chains continue in StateDev::sepx (HBM, grown by the host as the number of
// separation changes since the upload grows), so no length is refused.
constexpr int KSEP = 8;
constexpr int NSEPW = 2 + KSEP;

// HJ / TTR table in "cell-corner" layout: every grid cell stores the 2^ndim corner values
// it interpolates (lexicographic corner order, dim 0 slowest) contiguously, so one query
// reads 64 B (4-D) / 128 B (5-D) of values and 2^ndim * 16 * gw B of gradients -- one or
// two cache lines instead of 2^ndim scattered nodes. 16x the node table (1.8 GB for the
// full DI table): sized for 288 GB HBM, expanded on the device at upload.
struct TableDev {
  const float* cells;    // [n_cells][2^ndim]
  const float4* gcells;  // [n_cells][2^ndim][gw]
  int ndim;
  int n[5];        // nodes per dim
  int cstride[5];  // cell strides (cells per dim: n (periodic) or n - 1)
  float lo[5];
  float sp[5];
  float rsp[5];    // 1 / sp (float32, correctly rounded)
  int mdiv[5];     // 1: (s - lo) / sp by the reciprocal + one FMA correction (grid_pos), checked at
                   // upload to equal the division bit for bit over every float32 the lookups can
                   // meet (mdiv_check_kernel); 0: the division
  int periodic[5];
  int gw;  // float4 per corner gradient (1 for <= 4 dims, 2 for 5 dims)
  // Value bounds per block of 2^bshift cells per dim: (min, max) of the block's nodes widened
  // by the fp32 interpolation error (bounds_kernel). Small enough to stay in L2; the
  // workgroup kernel uses them to skip exact lookups that cannot be the argmin. nullptr: none.
  const float2* bnd;
  int bshift;
  int bstride[5];   // blocks: stride per dim
};

// Persistent per-env state: ONE contiguous record per env (env-major, 128-B aligned
// stride) whose byte layout is exactly the head of the env's LDS block (lds_plan), so a
// step starts with a straight float4 copy HBM -> LDS and ends with the copy back. Fields
// (16-B aligned each), in record order:
//   [0, a1)   ps [4][N], pdist, adiff [N] f64, done, reached, sfilt, decon [N] i32, step i32
//   [a1, a2)  cur [NCUR] + the HJ shift chain                               (reset only)
//   [a2, a3)  stats [NSTAT][N], winfo [NWINFO][N], gmt, minrel [N] f64
//   [a3, rec) lm [6][NL] f64 (x, y, heading, speed, sin, cos), lmd            (reset only)
// A step rewrites [0, a1) and [a2, a3). Everything a step needs before its distances is in
// [0, a2) (state, done flags, curriculum, shifts): the team kernel loads that part first and
// the rest while its agent wave filters and integrates (lsm_team.h).
struct StateDev {
  float4* rec;          // [n][rec_stride16]
  uint32_t rec_stride16;
  uint32_t rec16;       // float4 per record
  uint32_t a1_16, a2_16, a3_16;   // the boundaries above, in float4
  double* prev;         // [n][8] previous episode summary
  uint32_t* mt;         // [n][MT_WORDS] (LSM_RNG_PHILOX: only word MT_N, the reset index + MT_N)
  double* dep;          // [n][DEPW(N)] departed [N], departure_timer [N], init_theta [N], and the
                        // final disconnect mask of the last call (u64 bits) (LSM_SCENARIO_DEPARTURES)
  double* sepx;         // [n][sepx_cap] HJ separation shifts KSEP, KSEP + 1, ... of each env's chain
  uint32_t sepx_cap;    // (nullptr / 0 until a chain can outgrow the record's KSEP slots)
};

struct OutDev {
  float* obs;
  float* node;
  float* adj;
  float* rew;
  uint8_t* dones;
  uint8_t* reset_flag;
  double* ep_info;
  double* info;
  uint8_t* edges;
  double* state;
  uint64_t* adjmask;   // LSM_OUT_ADJ_MASK (compact adjacency layout)
  float* share_obs;    // LSM_OUT_SHARE_OBS (optional)
  float* masks;        // LSM_OUT_MASKS (optional)
  float* active_masks; // LSM_OUT_ACTIVE_MASKS (optional)
  double* cforce;      // LSM_OUT_COLLISION_FORCE (lsm_config.collision_forces only)
  uint8_t* departed;   // LSM_OUT_DEPARTED (optional)
  int64_t* adjnnz;     // LSM_OUT_ADJ_NNZ (optional): nonzeros of each ego's adjacency as stored
};

struct KParams {
  int n_envs, N, L, NL, E, F, OBS, dyn, episode_length, use_masking, use_filter_arg, auto_reset;
  int adj_compact;   // LSM_ADJ_COMPACT: unmasked E x E table once per env + per-ego masks
  int lean;          // the team kernel carves the lean LDS layout (lds_plan)
  int filter_search; // workgroup kernel's HJ argmin: 1 bound-pruned (default), 0 every pair exact
  int scenario;      // LSM_SCENARIO_*
  int rng;           // LSM_RNG_*
  int nis;           // World.num_internal_step (>= 1): filter -> integrate repeats per step
  int rbin;          // lsm_config.reward_terms (LSM_REWARD_* bits)
  int collab;        // lsm_config.collaborative: shared reward
  int rext;          // rbin || collab: rewards finished after every agent's goal / done update
  int use_hj;        // the HJ handle exists (filter on, or LSM_REWARD_HJ_VALUE): resets shift it
  int mt_stage;      // team-kernel resets: MT19937 words one lane may draw from the staged blocks
                     // (2 MT_N; lsm_test_set_mt_stage lowers it so tests reach the cooperative redraw)
  int64_t seed, env_offset;   // Philox keys: seed + 1000 * (env_offset + env)
  uint32_t lds_dep_off;       // LSM_SCENARIO_DEPARTURES: LDS offset of the departure arrays
  double dt, world_size, coord_range, world_eng, sep_target, max_speed, min_speed, gs_min, gs_max;
  double coord_range_s;  // the largest double s with sqrt(s) <= coord_range (correctly rounded sqrt):
                         // sqrt(s) > coord_range <=> s > coord_range_s, for squared distances s >= 0
  double scen_d2lo, scen_d2hi;   // the scenario's separated-positions band (dmin, dmax) on squared
                                 // distances: sqrt(s) > dmin <=> s > d2lo, sqrt(s) < dmax <=> s < d2hi
  double act0[5], act1[5];
  double mag_c[50], mag_s[50];
  double cos_pi6, two_pi, pi;
  double di_thr_xmax, di_thr_xmin, di_thr_ymax, di_thr_ymin, di_axmax, di_axmin, di_aymax, di_aymin;
  double at_vmax, at_vmin, at_amax, at_amin, at_wmax, at_thr_amax, at_thr_amin;
  float at_box_w, at_box_amax, at_box_amin;  // float32 box corners (jnp)
  double ttr_max;
  double val_sep0;       // separation of the uploaded value table (HjDataHandle.separation_distance)
  uint32_t m_E, m_EE, m_EF, m_F, m_EF4, m_NL;  // ceil(2^32 / d) for exact small-numerator division
  unsigned long long* stamps;     // LSM_OUT_DEBUG_STAMPS (diagnostic builds only)
  int diag;                       // diagnostic builds: bit 0 skip adj/node stores, bit 1 skip filter (LSM_DIAG)
  uint32_t lds_env_bytes;         // LDS bytes per env (envs per wave > 1: consecutive blocks)
  const uint16_t* pairs;          // strict upper-triangle entity pairs (a | b << 8)
  int32_t* action_err;            // set to 1 by a launch that saw an action index outside [0, 25)
  TableDev val, ttr;
  StateDev s;
  OutDev o;
};

// Per-launch kernel arguments (the rest lives in a device-resident KParams per handle).
struct KStep {
  const void* actions;
  const double* layout;   // mode 2: [n][layout doubles] (lsm_reset_layout)
  int action_kind, mode, emit_edges, stop_after;   // mode 0 = step, 1 = reset all, 2 = reset from layout
  double cur_new[NCUR];
};

__host__ __device__ inline size_t align16_(size_t x) { return (x + 15) & ~(size_t)15; }

// doubles per env of StateDev::dep: departed, timer, init_theta [N], then the accumulated
// disconnect mask of the step's last ego (the next update_graph's), up to 4 words (E <= 256)
__host__ __device__ inline int depw(int N) { return 3 * N + 4; }

// LDS bytes of the departure arrays (appended after lds_plan's block)
__host__ __device__ inline size_t dep_lds_bytes(int N) {
  return 3 * align16_(4 * (size_t)N) + 3 * align16_(8 * (size_t)N) + align16_(32 * (size_t)N);
}

struct LdsPlan {
  size_t bytes;     // LDS per env
  size_t rec;       // persistent record bytes (LDS head == HBM record)
  size_t a1, a2, a3;   // record sections (StateDev)
  size_t off[40];
};

// Workgroup-per-env kernel (lsm_block.h): threads per env and its limits.
constexpr int BT = 256;
constexpr int BMAXN = 64;
constexpr int BMAXE = 256;   // masks: E <= BT so one ballot per wave gives a mask word

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// The record's fields, in carve order: LdsPlan::off[REC_*] (host code; the device carves in order).
enum RecField { REC_PS = 0, REC_STATS, REC_WINFO, REC_PDIST, REC_GMT, REC_MINREL, REC_ADIFF, REC_DONE, REC_REACHED,
                REC_SFILT, REC_DECON, REC_STEP, REC_CUR, REC_LM, REC_LMD };

// Offsets of every LDS array (shared by the host launch/record init and the device carve).
// The record prefix (fields 0..14) is common to both kernels; the workgroup kernel keeps no
// landmark-distance cache (lmd, 0 bytes), no E x E / N x N tables, and adds the entity
// position table, per-ego multi-word masks and a node staging area.
__host__ __device__ inline LdsPlan lds_plan(int N, int NL, int E, int F, bool block = false,
                                            bool lean = false) {
  LdsPlan p;
  size_t o = 0;
  int k = 0;
  auto put = [&](size_t bytes) { p.off[k++] = o; o += align16(bytes); };
  // record: fields 0..14 (carve order: ps stats winfo pdist gmt minrel adiff done reached sfilt
  // decon step cur lm lmd) placed in the section order of StateDev
  {
    const size_t fsz[15] = {(size_t)8 * 4 * N, (size_t)8 * NSTAT * N, (size_t)8 * NWINFO * N, (size_t)8 * N,
                            (size_t)8 * N, (size_t)8 * N, (size_t)8 * N, (size_t)4 * N, (size_t)4 * N,
                            (size_t)4 * N, (size_t)4 * N, 8, (size_t)8 * (NCUR + NSEPW), (size_t)8 * 6 * NL,
                            block ? 0 : (size_t)4 * (NL * (NL - 1) / 2)};
    const int order[15] = {0, 3, 6, 7, 8, 9, 10, 11, 12, 1, 2, 4, 5, 13, 14};
#pragma unroll
    for (int q = 0; q < 15; ++q) {
      const int f = order[q];
      p.off[f] = o;
      o += align16(fsz[f]);
      if (f == 11) p.a1 = o;
      if (f == 12) p.a2 = o;
      if (f == 5) p.a3 = o;
    }
    k = 15;
  }
  p.rec = o;
  const int MW = (E + 63) / 64;
  // scratch
  put(4 * N); put(4 * N); put(8 * 2 * N); put(8 * 2 * N); put(8 * 2 * N); put(8 * 2 * N);
  put(block ? 8 * N * MW : 8 * N);
  put(F == 10 ? 0 : 8 * 2 * N);
  if (block) {
    // fval aa aa2 -> none; U1 = {mt, scen, scratch} | {feat, egooff} | {pair partials, info rows}
    put(8 * E); put(8 * E); put(4 * N); put(8 * 8);   // ex, ey, ccnt, mpre[4] + mpost[4]
    const size_t u1 = o;
    size_t c = align16(4 * MT_WORDS), d = c + align16(8 * SCEN_WS), e = d + align16(8 * 2 * N);
    size_t g1 = F == 10 ? align16(8 * (2 * N + NL) * F) : align16(8 * 4 * N);
    size_t g2 = g1 + (F == 10 ? align16(8 * N * F) : 0);
    size_t m = 8 * 2 * BT;
    m = m > (size_t)(8 * LSM_INFO_FIELDS * N) ? m : (size_t)(8 * LSM_INFO_FIELDS * N);
    size_t u1sz = e > g2 ? e : g2;
    u1sz = u1sz > align16(m) ? u1sz : align16(m);
    // the filter's per-wave survivor queues (lsm_block.h): (i, j) u16 + value f32 per slot
    const int tpe = (64 * N <= BT) ? 64 : (32 * N <= BT) ? 32 : (16 * N <= BT) ? 16 : (8 * N <= BT) ? 8 : 4;
    const size_t qb = align16((size_t)(BT / WAVE) * WAVE * ((N + tpe - 1) / tpe) * 6);
    u1sz = u1sz > qb ? u1sz : qb;
    p.off[k++] = u1; p.off[k++] = u1 + c; p.off[k++] = u1 + d;   // mt, scen, scratch
    p.off[k++] = u1; p.off[k++] = u1 + g1;                         // feat, egooff
    p.off[k++] = u1;                                               // dpair: pair partials / info rows
    o = u1 + u1sz;
    // node staging (airtaxi, or DI with E * F % 4 != 0): live together with feat
    const bool stage = F != 10 || ((E * F) & 3) != 0;
    p.off[k++] = o;
    o += stage ? align16(4 * BT * F) : 0;
    p.bytes = o;
    return p;
  }
  // U1
  const size_t u1 = o;
  const size_t fvb = lean ? (size_t)4 * (N * E + NL * N) : (size_t)4 * E * E;
  size_t a = align16(fvb), a2 = a + align16(8 * N * N), b = a2 + align16(8 * N * N);
  size_t c = align16(4 * MT_WORDS), d = c + align16(8 * SCEN_WS), e = d + align16(8 * 2 * MAXN);
  p.off[k++] = u1; p.off[k++] = u1 + a; p.off[k++] = u1 + a2; p.off[k++] = u1; p.off[k++] = u1 + c;
  p.off[k++] = u1 + d;
  size_t u1sz = b > e ? b : e;
  const size_t h0 = align16(4 * WAVE * F);   // node staging for up to 64 pairs
  u1sz = u1sz > h0 ? u1sz : h0;
  // pair matrices dpair, vpair, inr, then the team kernel's per-ego filter slots (filter_slot)
  size_t f1 = align16(8 * N * N), f2 = f1 + align16(8 * N * N), f3 = f2 + align16(N * N) + align16(32 * N);
  if (lean) u1sz = u1sz > f3 ? u1sz : f3;   // the pair matrices at the head of U1
  o = u1 + u1sz;
  // U2
  const size_t u2 = o;
  const size_t pb = lean ? u1 : u2;   // pair matrices
  // DI entity rows + ego offsets; airtaxi: the [4][N] heading trig table (feat) only
  size_t g1 = F == 10 ? align16(8 * (2 * N + NL) * F) : align16(8 * 4 * N);
  size_t g2 = g1 + (F == 10 ? align16(8 * N * F) : 0);
  p.off[k++] = pb; p.off[k++] = pb + f1; p.off[k++] = pb + f2;
  p.off[k++] = u2; p.off[k++] = u2 + g1; p.off[k++] = u1;   // stage aliases U1 (adj emitted first)
  size_t m = lean ? g2 : (f3 > g2 ? f3 : g2);
  // magnetic partials + the segment constants (DI, filter off; team kernel: mag_table_store)
  if (F == 10) m = m > (size_t)(8 * (2 * 64 + 100)) ? m : (size_t)(8 * (2 * 64 + 100));
  m = m > (size_t)(8 * LSM_INFO_FIELDS * N) ? m : (size_t)(8 * LSM_INFO_FIELDS * N);   // info rows
  // the next MT19937 block of a team-kernel reset (live with mt / scen; U2 is free then): after
  // U1's scratch when it fits, else at the U2 base (the team kernels' layouts have room either way,
  // lsm_create checks)
  const size_t mtb = align16(4 * MT_N);
  const bool mtn_u1 = u1sz - e >= mtb;
  p.off[k++] = mtn_u1 ? u1 + e : u2;
  if (!mtn_u1 && m < mtb) m = mtb;
  o = u2 + m;
  p.bytes = o;
  return p;
}

// The grid coordinate y / sp (y = s - lo in float32): the IEEE division, or -- where the upload check
// found them equal for every float32 y the lookups can meet -- q = y r, q + (y - q sp) r with
// r = 1 / sp (Markstein's correction, two FMAs instead of the ~10-instruction division sequence).
__host__ __device__ __forceinline__ float grid_pos(float y, float sp, float rsp, int mdiv) {
  if (!mdiv) return y / sp;
  const float q = y * rsp;
  const float r = fmaf(-q, sp, y);
  return fmaf(r, rsp, q);
}

// Env block stride for the team kernel: a multiple of 8 NT bytes with an odd quotient, so the
// 8-B per-agent fields of envs g = 0, 1, ... of one 32-lane ds_read_b64 group (256-B bank row)
// start on distinct bank offsets.
__host__ __device__ inline size_t team_env_bytes(size_t bytes, int N) {
  const size_t u = 8 * (size_t)N;
  size_t q = (bytes + u - 1) / u;
  if ((q & 1) == 0) ++q;
  return q * u;
}

}  // namespace lsm
