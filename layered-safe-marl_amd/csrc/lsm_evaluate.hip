// lsm_evaluate.hip -- the sequence form of the actor and critic heads (include/lsm_evaluate.h): a time-major
// minibatch of C chunks of T steps, the GRU state carried through each chunk's steps, the log-probability
// of the stored action, the entropy and the values.
//
// Reference: GR_Actor.evaluate_actions / GR_Critic.forward after gnn_base: MLPBase, the T x N branch of
// RNNLayer.forward (one nn.GRU call per run of steps between zero masks) and ACTLayer.evaluate_actions.
//
// Work split: lsm_policy.hip's, whose per-row pieces (csrc/lsm_head_tile.h) run here unchanged. A
// 256-thread workgroup owns 64 chunks, lane = chunk, its four waves split each layer's columns, and the
// tile walks its T steps: at step l its input rows l * C + b0 .. b0 + 63 are contiguous, so the loads are
// the one-step kernel's. The one-step kernel parks h in the input row, which the next step's inputs
// overwrite; here h of every GRU layer has an LDS row of its own for the whole call (recurrent_N more
// rows of pad(Hd) floats per chunk) and no state travels through global memory between steps. After a
// layer's cells each wave copies its own columns of h' from the activation row to the state row; the
// barriers of the following layers order that store before the next step's reads.
//
// Wave 0's lane walks its row's logits as the one-step kernel does (max; sum) and once more for the
// entropy, and keeps its chunk's two float64 dist_entropy sums in registers over the steps. At the end
// the 64 lanes' sums go through LDS to thread 0, which adds them in lane order and writes the group's pair
// to scratch; finish_kernel (one thread) adds the groups in order and divides.
//
// eval_tile is ONE __host__ __device__ text; lsm_host_head_evaluate runs it with a tile of one chunk and one
// "wave", and adds the chunks' sums in the kernel's grouping. Its step and copy loops stand here in full:
// eval_kernel is kept byte-identical, and reaching them through shared functions changes its code. Stage 1
// of lsm_backward.hip restates the step with saves; test_backwards_forward_is_evaluates holds the two to one.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsm_evaluate.h"
#include "lsm_head_tile.h"

namespace {

using namespace lsm_head_tile;

struct Eval : Shape {
  const float* w;
  lsm_eval_io io;
  int64_t C;
  int32_t T;
  int32_t SH;   // padded LDS row stride of a GRU state row
};

// One tile: chunks b0 .. b0 + rows - 1, lane = chunk (lane >= rows: an idle lane that keeps the barriers
// uniform and writes nothing), wave wv of nw; R = the tile's capacity in chunks (64 on the device, 1 on the
// host). part[0 .. 2): the tile's dist_entropy sums (entropy * weight, weight), written when
// io.dist_entropy is set. No path leaves before the last barrier.
LSM_HD void eval_tile(const Eval& n, const float* __restrict__ w, int64_t b0, int rows, int lane, int wv, int nw, int R,
                      float* lds, double* part) {
  const int tid = wv * R + lane, nt = nw * R;
  const int Hd = n.Hd, SX = n.SX, SA = n.SA, SH = n.SH, RN = n.RN, A = n.A;
  float* X = lds;
  float* cur = X + R * SX;
  float* nxt = cur + R * SA;
  float* H = nxt + R * SA;             // [RN][R][SH]: h of every GRU layer, for the whole call
  const bool active = lane < rows;
  const bool actor = n.kind == LSM_HEAD_ACTOR;
  float* xrow = X + lane * SX;
  const float* Wo = w + n.o_out;
  double acc_e = 0.0, acc_w = 0.0;

  for (int k = 0; k < RN; ++k)
    for (int i = tid; i < rows * Hd; i += nt) {
      const int r = i / Hd, c = i - r * Hd;
      H[(k * R + r) * SH + c] = n.io.rnn_states[((b0 + r) * RN + k) * Hd + c];
    }

  for (int l = 0; l < n.T; ++l) {
    const int64_t m0 = (int64_t)l * n.C + b0;   // the tile's first row of step l
    const int64_t m = m0 + lane;
    load_inputs(n, n.io.x0, n.io.x1, m0, rows, X, tid, nt);
    LSM_SYNC();
    mlp(n, w, xrow, cur + lane * SA, nxt + lane * SA, wv, nw);

    // ---- RNNLayer: h_k = h_k * mask, the GRU cells, h' kept for step l + 1 ---------------------------------
    for (int k = 0; k < RN; ++k) {
      float* Hk = H + k * R * SH;
      for (int i = tid; i < rows * Hd; i += nt) {
        const int r = i / Hd, c = i - r * Hd;
        Hk[r * SH + c] = Hk[r * SH + c] * n.io.masks[m0 + r];
      }
      LSM_SYNC();
      gru_layer(n, w, k, cur + lane * SA, Hk + lane * SH, nxt + lane * SA, wv, nw);
      LSM_SYNC();
      float* t = cur;
      cur = nxt;
      nxt = t;
      // this wave's columns of h': read by nobody before the next step's barriers
      for (int j0 = 4 * wv; j0 < Hd; j0 += 4 * nw)
        for (int j = j0; j < Hd && j < j0 + 4; ++j) Hk[lane * SH + j] = cur[lane * SA + j];
    }
    if (RN > 0) {
      layer_norm(cur + lane * SA, nxt + lane * SA, Hd, w + n.o_rn, w + n.o_rn + Hd, wv, nw);
      LSM_SYNC();
      float* t = cur;
      cur = nxt;
      nxt = t;
    }
    if (actor) {   // ACTLayer.evaluate_actions: x[isnan(x)] = 0, in place
      for (int i = tid; i < rows * Hd; i += nt) {
        const int r = i / Hd, c = i - r * Hd;
        const float v = cur[r * SA + c];
        if (!(v == v)) cur[r * SA + c] = 0.0f;
      }
      LSM_SYNC();
    }
    if (n.io.features)
      for (int i = tid; i < rows * Hd; i += nt) {
        const int r = i / Hd, c = i - r * Hd;
        n.io.features[m0 * Hd + i] = cur[r * SA + c];
      }

    // ---- the output layer ---------------------------------------------------------------------------------
    const float* feat = cur + lane * SA;
    if (!actor) {
      if (wv == 0 && active && n.io.values) {
        float v = Wo[Hd];
        for (int i = 0; i < Hd; ++i) v = fma_(Wo[i], feat[i], v);
        n.io.values[m] = v;
      }
      continue;   // the next step's first barrier keeps the other waves off this row until then
    }
    float* lg = nxt + lane * SA;
    linear(Wo, Wo + A * Hd, A, Hd, feat, lg, wv, nw, 0);
    LSM_SYNC();
    if (wv == 0 && active) {
      float mx, s;
      int first;
      masked_softmax(lg, A, n.io.available_actions ? n.io.available_actions + m * A : nullptr,
                     n.io.logits ? n.io.logits + m * A : nullptr, mx, first, s);
      bool bad;
      const int act = clamp_action(n.io.actions[m], A, bad);
      if (bad && n.io.bad) *n.io.bad = 1;
      const float ls = logf(s);
      if (n.io.log_probs) n.io.log_probs[m] = (lg[act] - mx) - ls;
      if (n.io.entropy || n.io.dist_entropy) {
        float sum = 0.0f;
        for (int a = 0; a < A; ++a) {
          const float d = lg[a] - mx;
          const float e = expf(d);
          if (e > 0.0f) sum += (e / s) * (d - ls);
        }
        const float ent = -sum;
        if (n.io.entropy) n.io.entropy[m] = ent;
        const double wt = n.io.active_masks ? (double)n.io.active_masks[m] : 1.0;
        acc_e += (double)ent * wt;
        acc_w += wt;
      }
    }
  }

  // ---- the state after the last step, and the tile's dist_entropy sums -----------------------------------
  LSM_SYNC();
  if (n.io.rnn_out)
    for (int k = 0; k < RN; ++k)
      for (int i = tid; i < rows * Hd; i += nt) {
        const int r = i / Hd, c = i - r * Hd;
        n.io.rnn_out[((b0 + r) * RN + k) * Hd + c] = H[(k * R + r) * SH + c];
      }
  if (actor && n.io.dist_entropy) {
    double* P = reinterpret_cast<double*>(X);   // 2 R doubles; an input row has at least 8 floats
    if (wv == 0) {
      P[2 * lane] = active ? acc_e : 0.0;
      P[2 * lane + 1] = active ? acc_w : 0.0;
    }
    LSM_SYNC();
    if (tid == 0) {
      double e = 0.0, wsum = 0.0;
      for (int r = 0; r < rows; ++r) e += P[2 * r], wsum += P[2 * r + 1];
      part[0] = e;
      part[1] = wsum;
    }
  }
}

// the groups' sums in order, one division, one rounding
LSM_HD void finish(const double* scratch, int64_t groups, float* dist_entropy) {
  double e = 0.0, wsum = 0.0;
  for (int64_t g = 0; g < groups; ++g) e += scratch[2 * g], wsum += scratch[2 * g + 1];
  *dist_entropy = (float)(e / wsum);
}

__global__ __launch_bounds__(BLOCK) void eval_kernel(Eval n, const float* __restrict__ w) {
  const Tile t = block_tile(n.C);
  eval_tile(n, w, t.row0, t.rows, t.lane, t.wv, WAVES, TILE, t.lds, n.io.scratch + 2 * (int64_t)blockIdx.x);
}

__global__ void finish_kernel(const double* scratch, int64_t groups, float* dist_entropy) {
  if (blockIdx.x == 0 && threadIdx.x == 0) finish(scratch, groups, dist_entropy);
}

int fail(const char* msg) { return refuse("evaluate: ", msg); }

size_t tile_floats(const Eval& n) { return (size_t)n.SX + 2 * (size_t)n.SA + (size_t)n.RN * n.SH; }

// the config's part of a call: the blob's layout, the LDS strides and the tile's LDS need; 0 when fine
int make_shape(const lsm_head_config& c, Eval* n) {
  if (layout(c, n, "evaluate: ") == 0) return 1;
  n->SH = pad(n->Hd);
  const size_t need = tile_bytes(tile_floats(*n));
  if (need > (size_t)WORKGROUP_LDS_BYTES) {
    char msg[200];
    snprintf(msg, sizeof msg,
             "the 64-chunk tile needs %zu bytes of LDS (input row %d, two activation rows %d, %d state rows %d "
             "floats), a workgroup has %d: use a smaller hidden or recurrent_N, or narrower inputs",
             need, n->SX, n->SA, n->RN, n->SH, WORKGROUP_LDS_BYTES);
    return fail(msg);
  }
  return 0;
}

int check_rows(int64_t C, int32_t T) { return check_sizes("evaluate: ", "C", "T * C", "minibatch", C, T); }

// every check of one call, shared by the device and the host entry point; fills n; 0 when fine
int make_eval(const lsm_head_config& c, const float* weights, const lsm_eval_io* io, int64_t C, int32_t T, Eval* n) {
  if (make_shape(c, n)) return 1;
  if (!weights) return fail("weights is null");
  if (!io) return fail("io is null");
  if (check_rows(C, T)) return 1;
  lsm_eval_io f = *io;
  drop_unread(*n, &f);
  if (n->RN == 0) f.rnn_out = nullptr;
  if (n->kind == LSM_HEAD_ACTOR) {
    f.values = nullptr;
  } else {
    f.actions = f.available_actions = f.active_masks = nullptr;
    f.log_probs = f.entropy = f.dist_entropy = f.logits = nullptr;
    f.scratch = nullptr;
  }
  const char* why = check_io(*n, weights, f, C,
                             {f.actions, f.available_actions, f.active_masks, f.log_probs, f.entropy, f.dist_entropy,
                              f.logits, f.values},
                             {f.bad, f.scratch}, "misaligned pointer (bad and scratch: 8 bytes)");
  if (why) return fail(why);
  if (n->kind == LSM_HEAD_ACTOR) {
    if (C > 0 && !f.actions) return fail("the actor needs actions");
    if (!f.log_probs && !f.entropy && !f.dist_entropy && !f.logits && !f.features && !f.rnn_out)
      return fail("the actor needs at least one output");
    if (f.dist_entropy && !f.scratch) return fail("dist_entropy needs scratch");
  }
  n->w = weights;
  n->io = f;
  n->C = C;
  n->T = T;
  return 0;
}

}  // namespace

int lsm_evaluate_fill_plan(const lsm_head_config& c, int64_t C, int32_t T, lsm_head_launch_plan* out) {
  Eval n;
  if (make_shape(c, &n) || check_rows(C, T)) return 1;
  out->SX = n.SX, out->SA = n.SA, out->SH = n.SH;
  out->lds_bytes[0] = (int64_t)tile_bytes(tile_floats(n));
  return 0;
}

extern "C" {

size_t lsm_head_evaluate_scratch_bytes(int64_t C, int32_t T) {
  if (C < 0 || T < 1) return 0;
  const int64_t g = tiles_of(C);
  return (size_t)(g < 1 ? 1 : g) * 2 * sizeof(double);
}

int lsm_head_evaluate(lsm_head_config cfg, const float* weights, const lsm_eval_io* io, int64_t C, int32_t T,
                      void* hip_stream) {
  Eval n;
  if (make_eval(cfg, weights, io, C, T, &n)) return 1;
  if (C == 0) return 0;
  // the LDS limit: to a workgroup's whole LDS
  const char* why = launch<eval_kernel, WORKGROUP_LDS_BYTES>((unsigned)tiles_of(C), BLOCK, tile_bytes(tile_floats(n)),
                                                             hip_stream, n, n.w);
  if (!why && n.io.dist_entropy)
    why = launch<finish_kernel>(1, 1, 0, hip_stream, (const double*)n.io.scratch, tiles_of(C), n.io.dist_entropy);
  return why ? fail(why) : 0;
}

int lsm_host_head_evaluate(lsm_head_config cfg, const float* weights, const lsm_eval_io* io, int64_t C, int32_t T) {
  Eval n;
  if (make_eval(cfg, weights, io, C, T, &n)) return 1;
  if (C == 0) return 0;
  std::vector<float4> lds(tile_floats(n) / 4 + 1);
  for (int64_t g = 0; g < tiles_of(C); ++g) {
    double e = 0.0, wsum = 0.0;   // the group's sums: its chunks in order, as the kernel's thread 0 adds its lanes
    for (int64_t b = g * TILE; b < C && b < (g + 1) * TILE; ++b) {
      double part[2] = {0.0, 0.0};
      eval_tile(n, n.w, b, 1, 0, 0, 1, 1, reinterpret_cast<float*>(lds.data()), part);
      e += part[0], wsum += part[1];
    }
    if (n.io.dist_entropy) n.io.scratch[2 * g] = e, n.io.scratch[2 * g + 1] = wsum;
  }
  if (n.io.dist_entropy) finish(n.io.scratch, tiles_of(C), n.io.dist_entropy);
  return 0;
}

}  // extern "C"
