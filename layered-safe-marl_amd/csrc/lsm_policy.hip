// lsm_policy.hip -- the actor and critic heads in one launch (include/lsm_policy.h).
//
// Reference: GR_Actor.forward / GR_Critic.forward after gnn_base (graph_actor_critic.py:162-172, 406-418):
// torch.cat, MLPBase (feature norm, fc1, fc2[i], a LayerNorm behind each), RNNLayer's one-step GRU with its
// norm, then ACTLayer's Categorical (mask, softmax, sample or mode, log-probability) or v_out: about two
// dozen small launches per network, nn.GRU and torch.multinomial among them. Here a row never leaves
// its workgroup: the two input blocks are read once into one LDS row, every activation lives in LDS, and
// only the outputs are written.
//
// Work split. A 256-thread workgroup owns a tile of 64 rows, lane = row; its four waves split each
// layer's output columns in blocks of four (wave w: blocks w, w + 4, ..). For one block a lane reads its
// row from LDS 16 bytes at a time and runs 16 FMAs per read, the weights lane-uniform through the scalar
// cache (four weight rows, scalar operands of the FMAs). Each Linear writes its activated outputs to the
// other activation buffer; after a barrier every thread computes its row's LayerNorm statistics (the
// same order in every wave, so the four waves hold the same bits) and writes its own columns back to the
// first buffer; one more barrier. A GRU layer stages h = state * mask of the tile into LDS, then runs six
// dot products per hidden unit (W_i{r,z,n} x, W_h{r,z,n} h) and the gate arithmetic in the owning lane;
// h' goes to LDS and, after the layer's barrier, from there to rnn_out, consecutive threads writing
// consecutive floats (as features is written). The weight blob is a __restrict__ kernel argument of its
// own, so these stores do not keep the later layers' weight loads off the scalar cache. The
// actor's logits go through LDS to wave 0, whose lane walks its row's num_actions entries in ascending
// order three times (max; sum; running sum against u * s). Every sum runs in one lane in a fixed order (four
// partial sums over the inputs i mod 4, each ascending, see dot4): no atomics, no cross-lane reduction,
// bit-reproducible.
//
// LDS (floats per tile row): the input row pad(max(in, Hd)) (h lives there during the GRU) and two
// activation rows pad(max(Hd, A)), pad(w) = round_up(w, 4) + 4: 16-byte aligned rows whose stride is not a
// multiple of 64 banks (lane r's row starts 4 (r mod 16) banks on for width 64).
//
// tile_forward is ONE __host__ __device__ text; lsm_host_head_forward runs it with a tile of one row and
// one "wave". The kernel's entry, the tile-row copies, the per-row pieces (dot4, linear, layer_norm, MLPBase,
// the GRU cells, the softmax walks), the config's and the call's checks and launch() live in lsm_head_tile.h,
// which lsm_evaluate.hip and lsm_backward.hip run too.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsm_policy.h"
#include "lsm_head_tile.h"   // the pieces shared with lsm_evaluate.hip and lsm_backward.hip

namespace {

using namespace lsm_head_tile;

struct Head : Shape {
  const float* w;
  lsm_head_io io;
  int64_t M;
};

// One tile: rows row0 .. row0 + rows - 1, lane = row (lane >= rows: an idle lane that keeps the barriers
// uniform and writes nothing), wave wv of nw; R = the tile's capacity in rows (64 on the device, 1 on the host).
// w is the weight blob as a parameter of its own: as a __restrict__ kernel argument it is known not to alias
// the outputs, so the stores between the layers do not stop its loads from going through the scalar cache.
LSM_HD void tile_forward(const Head& n, const float* __restrict__ w, int64_t row0, int rows, int lane, int wv, int nw,
                         int R, float* lds) {
  const int tid = wv * R + lane, nt = nw * R;
  const int Hd = n.Hd, SX = n.SX, SA = n.SA, RN = n.RN;
  float* X = lds;
  float* cur = X + R * SX;
  float* nxt = cur + R * SA;
  const bool active = lane < rows;
  const int64_t m = row0 + lane;
  float* xrow = X + lane * SX;

  // ---- the virtual cat([x0, x1]), the feature norm and MLPLayer --------------------------------------------
  load_inputs(n, n.io.x0, n.io.x1, row0, rows, X, tid, nt);
  LSM_SYNC();
  mlp(n, w, xrow, cur + lane * SA, nxt + lane * SA, wv, nw);

  // ---- RNNLayer: recurrent_N GRU cells on h = state * mask, then its norm --------------------------------
  for (int l = 0; l < RN; ++l) {
    load_rows(X, SX, Hd, n.io.rnn_states + l * Hd, row0, rows, tid, nt, (RN - 1) * Hd, TimesRow{n.io.masks, row0});
    LSM_SYNC();
    gru_layer(n, w, l, cur + lane * SA, xrow, nxt + lane * SA, wv, nw);
    LSM_SYNC();
    float* c = cur;
    cur = nxt;
    nxt = c;
    // h'_l of the tile, from LDS
    if (n.io.rnn_out) save_rows(cur, SA, Hd, n.io.rnn_out + l * Hd, row0, rows, tid, nt, (RN - 1) * Hd);
  }
  if (RN > 0) {
    layer_norm(cur + lane * SA, nxt + lane * SA, Hd, w + n.o_rn, w + n.o_rn + Hd, wv, nw);
    LSM_SYNC();
    float* c = cur;
    cur = nxt;
    nxt = c;
  }
  if (n.io.features) save_rows(cur, SA, Hd, n.io.features, row0, rows, tid, nt);

  // ---- the output layer -------------------------------------------------------------------------------------
  const float* Wo = w + n.o_out;
  const float* feat = cur + lane * SA;
  if (n.kind == LSM_HEAD_CRITIC) {
    if (wv == 0 && active && n.io.values) {
      float v = Wo[Hd];
      for (int i = 0; i < Hd; ++i) v = fma_(Wo[i], feat[i], v);
      n.io.values[m] = v;
    }
    return;
  }
  const int A = n.A;
  float* lg = nxt + lane * SA;
  linear(Wo, Wo + A * Hd, A, Hd, feat, lg, wv, nw, 0);
  LSM_SYNC();
  if (wv != 0 || !active) return;
  float mx, s;
  int first;
  masked_softmax(lg, A, n.io.available_actions ? n.io.available_actions + m * A : nullptr,
                 n.io.logits ? n.io.logits + m * A : nullptr, mx, first, s);
  int pick = first;
  if (n.io.u) {
    float u = n.io.u[m];
    if (!(u >= 0.0f && u < 1.0f)) {
      if (n.io.bad) *n.io.bad = 1;
      u = u >= 1.0f ? 0.99999994f : 0.0f;   // NaN and negatives: 0
    }
    const float thr = u * s;
    float run = 0.0f;
    int last = -1;
    pick = -1;
    for (int a = 0; a < A; ++a) {
      const float e = expf(lg[a] - mx);
      run += e;
      if (e > 0.0f) last = a;
      if (pick < 0 && run > thr) pick = a;
    }
    if (pick < 0) pick = last < 0 ? 0 : last;
  }
  if (n.io.actions_i32) n.io.actions_i32[m] = pick;
  if (n.io.actions_f32) n.io.actions_f32[m] = (float)pick;
  if (n.io.log_probs) n.io.log_probs[m] = (lg[pick] - mx) - logf(s);
}

__global__ __launch_bounds__(BLOCK) void head_kernel(Head n, const float* __restrict__ w) {
  const Tile t = block_tile(n.M);
  tile_forward(n, w, t.row0, t.rows, t.lane, t.wv, WAVES, TILE, t.lds);
}

thread_local char g_err[256];

int fail(const char* msg) { return refuse("head: ", msg); }

// the largest tile the limits allow (in = 256, hidden = 128): 134144 bytes, within one workgroup's 160 KB
constexpr int MAX_TILE_BYTES = TILE * (pad(MAX_IN) + 2 * pad(MAX_HIDDEN)) * (int)sizeof(float);
static_assert(MAX_TILE_BYTES <= WORKGROUP_LDS_BYTES, "the worst-case tile must fit one workgroup's LDS");

int check_rows(int64_t M, int32_t T) { return check_sizes("head: ", "M", "M", "batch", M, T); }

// the tile's LDS floats per row: the input row and two activation rows
size_t tile_floats(const Shape& n) { return (size_t)n.SX + 2 * (size_t)n.SA; }

// every check of one call, shared by the device and the host entry point; fills n; 0 when fine
int make_head(const lsm_head_config& c, const float* weights, const lsm_head_io* io, int64_t M, Head* n) {
  if (layout(c, n, "head: ") == 0) return 1;
  if (!weights) return fail("weights is null");
  if (!io) return fail("io is null");
  if (check_rows(M, 1)) return 1;
  lsm_head_io f = *io;
  drop_unread(*n, &f);
  if (n->RN == 0) f.rnn_out = nullptr;
  if (n->kind == LSM_HEAD_ACTOR) {
    f.values = nullptr;
  } else {
    f.u = f.available_actions = nullptr;
    f.actions_i32 = nullptr;
    f.actions_f32 = f.log_probs = f.logits = nullptr;
  }
  const char* why = check_io(*n, weights, f, M,
                             {f.u, f.available_actions, f.actions_i32, f.actions_f32, f.log_probs, f.logits, f.values},
                             {f.bad}, "misaligned pointer");
  if (why) return fail(why);
  if (n->kind == LSM_HEAD_ACTOR && !f.actions_i32 && !f.actions_f32)
    return fail("the actor needs actions_i32 or actions_f32");
  n->w = weights;
  n->io = f;
  n->M = M;
  return 0;
}

}  // namespace

void lsm_policy_set_error(const char* prefix, const char* msg) {
  snprintf(g_err, sizeof g_err, "%s%s", prefix, msg);
}

extern "C" {

const char* lsm_policy_last_error(void) { return g_err; }

size_t lsm_head_weights_floats(lsm_head_config cfg) {
  Shape n;
  return layout(cfg, &n, "head: ");
}

int lsm_head_plan(lsm_head_config cfg, int32_t which, int64_t C, int32_t T, lsm_head_launch_plan* out) {
  if (!out) return lsm_policy_set_error("plan: ", "out is null"), 1;
  lsm_head_launch_plan p = {};
  if (which == LSM_HEAD_PLAN_FORWARD) {
    Shape n;
    if (layout(cfg, &n, "head: ") == 0) return 1;
    if (check_rows(C, T)) return 1;
    const size_t lds = tile_bytes(tile_floats(n));
    if (lds > (size_t)MAX_TILE_BYTES) return fail("the tile exceeds the LDS of one workgroup");
    p.SX = n.SX, p.SA = n.SA;
    p.lds_bytes[0] = (int64_t)lds;
  } else if (which == LSM_HEAD_PLAN_EVALUATE) {
    if (lsm_evaluate_fill_plan(cfg, C, T, &p)) return 1;
  } else if (which == LSM_HEAD_PLAN_BACKWARD) {
    if (lsm_backward_fill_plan(cfg, C, T, &p)) return 1;
  } else {
    return lsm_policy_set_error("plan: ", "unknown routine"), 1;
  }
  *out = p;
  return 0;
}

int lsm_head_forward(lsm_head_config cfg, const float* weights, const lsm_head_io* io, int64_t M, void* hip_stream) {
  Head n;
  if (make_head(cfg, weights, io, M, &n)) return 1;
  if (M == 0) return 0;
  const size_t lds = tile_bytes(tile_floats(n));
  if (lds > (size_t)MAX_TILE_BYTES) return fail("the tile exceeds the LDS of one workgroup");
  // the LDS limit: to the limits' worst case
  const char* why = launch<head_kernel, MAX_TILE_BYTES>((unsigned)tiles_of(M), BLOCK, lds, hip_stream, n, n.w);
  return why ? fail(why) : 0;
}

int lsm_host_head_forward(lsm_head_config cfg, const float* weights, const lsm_head_io* io, int64_t M) {
  Head n;
  if (make_head(cfg, weights, io, M, &n)) return 1;
  std::vector<float4> scratch(tile_floats(n) / 4 + 1);
  for (int64_t m = 0; m < M; ++m) tile_forward(n, n.w, m, 1, 0, 0, 1, 1, reinterpret_cast<float*>(scratch.data()));
  return 0;
}

}  // extern "C"
