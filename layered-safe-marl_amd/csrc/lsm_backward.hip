// lsm_backward.hip -- the backward pass through the actor and critic heads (include/lsm_backward.h): BPTT
// through the GRU, the gradient at the two input blocks and the gradient of every packed weight, from the
// loss's gradient at the logits or the values.
//
// Three stages on the stream, all built from ONE __host__ __device__ text each; lsm_host_head_backward runs
// them with a tile of one chunk and one "wave", and the same slab grouping.
//
// Stage 1, fwd_tile: lsm_evaluate.hip's eval_tile without the output layer (the seeds are given), with the
// pieces of csrc/lsm_head_tile.h (mlp and gru_layer through the hook Saves), and with saves. A 256-thread
// workgroup owns 64 chunks, lane = chunk, its four waves split each layer's columns, and the tile walks l =
// 0 .. T - 1. What a whole LDS row holds after a barrier (the input of fc1, every activation and LayerNorm
// output, the masked state, h', the features) is copied to workspace coalesced by all threads; the GRU's gates
// are written by the thread that computed them (16 bytes per lane and column block).
//
// Stage 2, bwd_tile: same ownership, l = T - 1 .. 0. Per chunk in LDS: B0 (a staged saved row, or the GRU's
// four gate gradients E), B1 (a gradient row as wide as the input), B2 (a gradient row of Hd) and the state's
// gradient dH of every GRU layer, which never leaves the workgroup. The transposed products W^T delta are
// tdot4, dot4's mirror image: the four outputs of a block of inputs accumulate over j ascending, one chain
// each, from lane-uniform weight reads. Elementwise work (the gates, the activations) is done by the thread
// that owns the column, reading the saved values of its own row and column straight from workspace. Every
// Linear's pre-activation gradient and every LayerNorm's (dy * xhat, dy) pair goes to workspace.
//
// Stage 3, dw_thread / finish_entry: every weight gradient is a job "out[j][i] = sum_m d[m][j] * x[m][i],
// i <= nin, with x[m][nin] = 1" (the bias column; the LayerNorm vectors are jobs with nin == 0). A workgroup
// takes one slab of LSM_BWD_SLAB rows and one 64 x 64 tile of a job, a thread 4 x 4 entries, each summed
// over the slab's rows ascending in float32 (three levels of 16, 16 and 8; the bias column with two-sum); the
// slab's partial blob goes to workspace and a last launch adds the slabs in ascending order in float64.
//
// Workspace layout (Bwd's o_* offsets, in floats, all int64): arrays of [R][n] in the order of
// include/lsm_backward.h, then the slabs' partial blobs.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsm_backward.h"
#include "lsm_head_tile.h"

namespace {

using namespace lsm_head_tile;

constexpr int SLAB = LSM_BWD_SLAB;
constexpr int DW_TILE = 64;    // a stage-3 workgroup's tile of a job: 64 x 64 entries, 4 x 4 per thread
constexpr int DW_RUN = 16;     // rows per FMA chain, and runs per middle sum, within a slab
constexpr int MAX_JOBS = 1 + 2 * (MAX_LAYERS + 1) + 2 * MAX_RNN + 1 + 1;

// out[j][i] = sum_m d[m][j] * x[m][i] (i < nin: to w + j * nin + i) and sum_m d[m][j] (to b + j)
struct Job {
  int64_t d, x;          // workspace offsets of the [R][nout] and [R][nin] arrays
  int32_t nout, nin;
  int32_t w, b;          // offsets in the blob
  int32_t tile0, ti_n;   // the job's first tile, its tiles along i
};

struct Bwd : Shape {
  const float* w;
  lsm_bwd_io io;
  int64_t C, R, NW, slabs;
  int32_t T, SH, HP, S0, S1, S2;
  int64_t o_u0, o_p[MAX_LAYERS + 1], o_y[MAX_LAYERS + 1];
  int64_t o_hm[MAX_RNN], o_r[MAX_RNN], o_z[MAX_RNN], o_g[MAX_RNN], o_hg[MAX_RNN], o_ho[MAX_RNN], o_feat;
  int64_t o_dout, o_vr, o_di[MAX_RNN], o_dh[MAX_RNN], o_v[MAX_LAYERS + 1], o_dl[MAX_LAYERS + 1], o_vf, o_part;
  int64_t ws_floats;
  int32_t njobs, ntiles;
  Job job[MAX_JOBS];
};

// ---- stage 1: the forward with saves ------------------------------------------------------------------------

// mlp's and gru_layer's hook for the tile's rows m0 ..: rows of X, nxt or cur to their [R][width] array of
// the workspace, coalesced; the gates to theirs by the thread that computed them (an idle lane writes nothing)
struct Saves {
  const Bwd& n;
  float* ws;
  const float *X, *cur, *nxt;   // the tile's buffers as mlp sees them
  int64_t m0;
  int nrows, lane, tid, nt;
  // the array's row m0 is the base, so that the index in the copy loop is the 32-bit i alone
  LSM_HD void save(int64_t at, const float* tile, int stride, int width) const {
    save_rows(tile, stride, width, ws + at + m0 * width, 0, nrows, tid, nt);
  }
  LSM_HD void rows(Saved which, int k) const {
    if (which == SAVED_INPUT) save(n.o_u0, X, n.SX, n.in);
    if (which == SAVED_ACT) save(n.o_p[k], nxt, n.SA, n.Hd);
    if (which == SAVED_NORM) save(n.o_y[k], cur, n.SA, n.Hd);
  }
  LSM_HD void gates(int k, int j, float r, float z, float g, float hg) const {
    if (lane >= nrows) return;
    const int64_t at = (m0 + lane) * n.Hd + j;
    ws[n.o_r[k] + at] = r, ws[n.o_z[k] + at] = z, ws[n.o_g[k] + at] = g, ws[n.o_hg[k] + at] = hg;
  }
};

// One tile, eval_tile's arguments and LDS
LSM_HD void fwd_tile(const Bwd& n, const float* __restrict__ w, int64_t b0, int rows, int lane, int wv, int nw, int R,
                     float* lds) {
  const int tid = wv * R + lane, nt = nw * R;
  const int Hd = n.Hd, SX = n.SX, SA = n.SA, SH = n.SH, RN = n.RN;
  float* X = lds;
  float* cur = X + R * SX;
  float* nxt = cur + R * SA;
  float* H = nxt + R * SA;   // [RN][R][SH]

  for (int k = 0; k < RN; ++k)
    load_rows(H + k * R * SH, SH, Hd, n.io.rnn_states + k * Hd, b0, rows, tid, nt, (RN - 1) * Hd);

  for (int l = 0; l < n.T; ++l) {
    const int64_t m0 = (int64_t)l * n.C + b0;
    const Saves keep{n, static_cast<float*>(n.io.workspace), X, cur, nxt, m0, rows, lane, tid, nt};
    load_inputs(n, n.io.x0, n.io.x1, m0, rows, X, tid, nt);
    LSM_SYNC();
    mlp(n, w, X + lane * SX, cur + lane * SA, nxt + lane * SA, wv, nw, keep);
    for (int k = 0; k < RN; ++k) {
      float* Hk = H + k * R * SH;
      load_rows(Hk, SH, Hd, Hk, 0, rows, tid, nt, SH - Hd, TimesRow{n.io.masks, m0});   // h_k *= mask
      LSM_SYNC();
      keep.save(n.o_hm[k], Hk, SH, Hd);
      gru_layer(n, w, k, cur + lane * SA, Hk + lane * SH, nxt + lane * SA, wv, nw, keep);
      LSM_SYNC();
      float* t = cur;
      cur = nxt;
      nxt = t;
      for (int j0 = 4 * wv; j0 < Hd; j0 += 4 * nw)
        for (int j = j0; j < Hd && j < j0 + 4; ++j) Hk[lane * SH + j] = cur[lane * SA + j];
      keep.save(n.o_ho[k], cur, SA, Hd);
    }
    if (RN > 0) {
      layer_norm(cur + lane * SA, nxt + lane * SA, Hd, w + n.o_rn, w + n.o_rn + Hd, wv, nw);
      float* t = cur;
      cur = nxt;
      nxt = t;
    }
    LSM_SYNC();   // the LayerNorm's rows are whole, and every save of cur above is done
    if (n.kind == LSM_HEAD_ACTOR) {   // ACTLayer.evaluate_actions: x[isnan(x)] = 0, in place
      for (int i = tid; i < rows * Hd; i += nt) {
        const int r = i / Hd, c = i - r * Hd;
        const float v = cur[r * SA + c];
        if (!(v == v)) cur[r * SA + c] = 0.0f;
      }
      LSM_SYNC();
    }
    keep.save(n.o_feat, cur, SA, Hd);
    // the next step writes cur only after two barriers
  }
}

// ---- stage 2: the backward sweep ----------------------------------------------------------------------------

// acc[c] += sum over j < nrows, ascending, of W[j * ld + c] * d[j] for c < nc <= 4 (the other accumulators
// follow column 0 and are dropped by the caller): dot4's mirror image, one FMA chain per output, a
// lane-uniform read of four adjacent weights per j. d is a 16-byte aligned LDS row.
LSM_HD void tdot4(const float* __restrict__ W, int ld, int nrows, int nc, const float* d, float (&acc)[4]) {
  const int c1 = nc > 1 ? 1 : 0, c2 = nc > 2 ? 2 : 0, c3 = nc > 3 ? 3 : 0;
  int j = 0;
  for (; j + 4 <= nrows; j += 4) {
    const float4 v = *reinterpret_cast<const float4*>(d + j);
    const float dv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const float* __restrict__ wr = W + (int64_t)(j + jj) * ld;
      acc[0] = fma_(wr[0], dv[jj], acc[0]);
      acc[1] = fma_(wr[c1], dv[jj], acc[1]);
      acc[2] = fma_(wr[c2], dv[jj], acc[2]);
      acc[3] = fma_(wr[c3], dv[jj], acc[3]);
    }
  }
  for (; j < nrows; ++j) {
    const float* __restrict__ wr = W + (int64_t)j * ld;
    const float dj = d[j];
    acc[0] = fma_(wr[0], dj, acc[0]);
    acc[1] = fma_(wr[c1], dj, acc[1]);
    acc[2] = fma_(wr[c2], dj, acc[2]);
    acc[3] = fma_(wr[c3], dj, acc[3]);
  }
}

// The backward of y = LayerNorm(n)(p) followed by the backward of p = act(a), in place: dy's row holds the
// gradient at y on entry and the gradient at a on return (act: 0 none, 1 ReLU, 2 Tanh). p: the LayerNorm's
// input row. nanzero: y's NaN entries were zeroed by the actor's rule and get gradient 0. V (row m's 2 n
// floats, or null): dy * xhat, dy, the terms of dgamma / dbeta; dl (row m's n floats, or null): the result.
// The statistics run over the whole row in every wave, in the same order; the wave's own column blocks are
// written after the barrier inside. The caller's barrier follows.
LSM_HD void ln_act_bwd(const float* p, float* dy, int n, const float* __restrict__ gamma, const float* __restrict__ beta,
                       bool nanzero, int act, float* V, float* dl, int wv, int nw) {
  const float mean = row_sum(p, n, 0.0f, false) / (float)n;
  const float rs = rsq_(row_sum(p, n, mean, true) / (float)n + 1e-5f);
  float s1 = 0.0f, s2 = 0.0f;
  for (int j = 0; j < n; ++j) {
    const float xh = (p[j] - mean) * rs;
    float d = dy[j];
    if (nanzero) {
      const float y = fma_(xh, gamma[j], beta[j]);
      if (!(y == y)) d = 0.0f;
    }
    const float g = d * gamma[j];
    s1 += g;
    s2 = fma_(g, xh, s2);
  }
  const float m1 = s1 / (float)n, m2 = s2 / (float)n;
  LSM_SYNC();
  for (int j0 = 4 * wv; j0 < n; j0 += 4 * nw)
    for (int j = j0; j < n && j < j0 + 4; ++j) {
      const float pj = p[j];
      const float xh = (pj - mean) * rs;
      float d = dy[j];
      if (nanzero) {
        const float y = fma_(xh, gamma[j], beta[j]);
        if (!(y == y)) d = 0.0f;
      }
      if (V) V[j] = d * xh, V[n + j] = d;
      float dp = rs * ((d * gamma[j] - m1) - xh * m2);
      if (act == 1)
        dp = pj > 0.0f ? dp : 0.0f;
      else if (act == 2)
        dp = dp * (1.0f - pj * pj);
      dy[j] = dp;
      if (dl) dl[j] = dp;
    }
}

LSM_HD void bwd_tile(const Bwd& n, const float* __restrict__ w, int64_t b0, int rows, int lane, int wv, int nw, int R,
                     float* lds) {
  const int tid = wv * R + lane, nt = nw * R;
  const int Hd = n.Hd, HP = n.HP, S0 = n.S0, S1 = n.S1, S2 = n.S2, SH = n.SH, RN = n.RN, A = n.A, in = n.in;
  float* ws = static_cast<float*>(n.io.workspace);
  float* B0 = lds;
  float* B1 = B0 + R * S0;
  float* B2 = B1 + R * S1;
  float* dH = B2 + R * S2;   // [RN][R][SH]: the gradient at every GRU layer's state, carried to step l - 1
  const bool active = lane < rows;
  const bool actor = n.kind == LSM_HEAD_ACTOR;
  float* b0r = B0 + lane * S0;
  float* b1r = B1 + lane * S1;
  float* b2r = B2 + lane * S2;
  const float* Wo = w + n.o_out;

  for (int k = 0; k < RN; ++k)
    for (int i = tid; i < R * SH; i += nt) dH[k * R * SH + i] = 0.0f;
  LSM_SYNC();

  for (int l = n.T - 1; l >= 0; --l) {
    const int64_t m0 = (int64_t)l * n.C + b0;
    const int64_t m = m0 + lane;
    const int64_t mr = active ? m : m0;   // the row an idle lane reads in its place; it writes nothing

    // ---- the output layer: delta_out, dfeatures = W_out^T delta_out into B2 -------------------------------
    if (actor) {
      for (int i = tid; i < rows * A; i += nt) {
        const int r = i / A, c = i - r * A;
        float v = n.io.dlogits[m0 * A + i];
        if (n.io.available_actions && n.io.available_actions[m0 * A + i] == 0.0f) v = 0.0f;
        B1[r * S1 + c] = v;
        ws[n.o_dout + m0 * A + i] = v;
      }
      LSM_SYNC();
      for (int i0 = 4 * wv; i0 < Hd; i0 += 4 * nw) {
        const int nc = Hd - i0 < 4 ? Hd - i0 : 4;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        tdot4(Wo + i0, Hd, A, nc, b1r, acc);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < nc) b2r[i0 + c] = acc[c];
      }
    } else {
      for (int i = tid; i < rows; i += nt) ws[n.o_dout + m0 + i] = n.io.dvalues[m0 + i];
      const float dv = n.io.dvalues[mr];
      for (int i0 = 4 * wv; i0 < Hd; i0 += 4 * nw)
        for (int i = i0; i < Hd && i < i0 + 4; ++i) b2r[i] = Wo[i] * dv;
    }
    LSM_SYNC();

    // ---- the RNN's LayerNorm, then the GRU layers from the top ---------------------------------------------
    if (RN > 0) {
      load_rows(B0, S0, Hd, ws + n.o_ho[RN - 1], m0, rows, tid, nt);
      LSM_SYNC();
      ln_act_bwd(b0r, b2r, Hd, w + n.o_rn, w + n.o_rn + Hd, actor, 0, active ? ws + n.o_vr + m * 2 * Hd : nullptr,
                 nullptr, wv, nw);
      LSM_SYNC();
    }
    for (int k = RN - 1; k >= 0; --k) {
      float* dHk = dH + (k * R + lane) * SH;
      const float* Wih = w + n.o_gru[k];
      const float* Whh = Wih + 3 * Hd * Hd;
      const float mask = n.io.masks[mr];
      // the cell's elementwise backward on this thread's columns: E = [dr_pre, dz_pre, dn_pre, dn_pre * r]
      // into B0 (sections of HP floats), dh * z into B2
      for (int j0 = 4 * wv; j0 < Hd; j0 += 4 * nw)
        for (int j = j0; j < Hd && j < j0 + 4; ++j) {
          const int64_t at = mr * Hd + j;
          const float r = ws[n.o_r[k] + at], z = ws[n.o_z[k] + at], g = ws[n.o_g[k] + at];
          const float hg = ws[n.o_hg[k] + at], hm = ws[n.o_hm[k] + at];
          const float dh = b2r[j] + dHk[j];
          const float dgp = (dh * (1.0f - z)) * (1.0f - g * g);
          const float drp = (dgp * hg) * (r * (1.0f - r));
          const float dzp = (dh * (hm - g)) * (z * (1.0f - z));
          const float dhg = dgp * r;
          b0r[j] = drp, b0r[HP + j] = dzp, b0r[2 * HP + j] = dgp, b0r[3 * HP + j] = dhg;
          b2r[j] = dh * z;
          if (active) {
            float* di = ws + n.o_di[k] + m * 3 * Hd;
            float* dhh = ws + n.o_dh[k] + m * 3 * Hd;
            di[j] = drp, di[Hd + j] = dzp, di[2 * Hd + j] = dgp;
            dhh[j] = drp, dhh[Hd + j] = dzp, dhh[2 * Hd + j] = dhg;
          }
        }
      LSM_SYNC();
      for (int i0 = 4 * wv; i0 < Hd; i0 += 4 * nw) {
        const int nc = Hd - i0 < 4 ? Hd - i0 : 4;
        float ax[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ah[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        tdot4(Wih + i0, Hd, Hd, nc, b0r, ax);
        tdot4(Wih + Hd * Hd + i0, Hd, Hd, nc, b0r + HP, ax);
        tdot4(Wih + 2 * Hd * Hd + i0, Hd, Hd, nc, b0r + 2 * HP, ax);
        tdot4(Whh + i0, Hd, Hd, nc, b0r, ah);
        tdot4(Whh + Hd * Hd + i0, Hd, Hd, nc, b0r + HP, ah);
        tdot4(Whh + 2 * Hd * Hd + i0, Hd, Hd, nc, b0r + 3 * HP, ah);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < nc) {
            b1r[i0 + c] = ax[c];
            dHk[i0 + c] = (b2r[i0 + c] + ah[c]) * mask;   // h = h * mask: dh_prev = dh * mask
          }
      }
      LSM_SYNC();
      // the layer's input gradient: the layer below's dh of this step, or the gradient at the MLP's output
      for (int j0 = 4 * wv; j0 < Hd; j0 += 4 * nw)
        for (int j = j0; j < Hd && j < j0 + 4; ++j) b2r[j] = b1r[j];
    }

    // ---- MLPBase from its last layer ------------------------------------------------------------------------
    for (int k = n.L; k >= 0; --k) {
      const int din = k == 0 ? in : Hd;
      const float* W = w + n.o_fc[k];
      const float* b = W + Hd * din;
      load_rows(B0, S0, Hd, ws + n.o_p[k], m0, rows, tid, nt);
      LSM_SYNC();
      ln_act_bwd(b0r, b2r, Hd, b + Hd, b + 2 * Hd, actor && RN == 0 && k == n.L, n.relu ? 1 : 2,
                 active ? ws + n.o_v[k] + m * 2 * Hd : nullptr, active ? ws + n.o_dl[k] + m * Hd : nullptr, wv, nw);
      LSM_SYNC();
      for (int i0 = 4 * wv; i0 < din; i0 += 4 * nw) {
        const int nc = din - i0 < 4 ? din - i0 : 4;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        tdot4(W + i0, din, Hd, nc, b2r, acc);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < nc) b1r[i0 + c] = acc[c];
      }
      LSM_SYNC();
      if (k > 0)
        for (int j0 = 4 * wv; j0 < Hd; j0 += 4 * nw)
          for (int j = j0; j < Hd && j < j0 + 4; ++j) b2r[j] = b1r[j];
    }

    // ---- the feature norm, and the gradient at the two input blocks ------------------------------------------
    if (n.fnorm) {
      load_rows(B0, S0, n.in0, n.io.x0, m0, rows, tid, nt);   // the virtual cat([x0, x1]) again
      load_rows(B0 + n.in0, S0, n.in1, n.io.x1, m0, rows, tid, nt);
      LSM_SYNC();
      ln_act_bwd(b0r, b1r, in, w + n.o_fn, w + n.o_fn + in, false, 0, active ? ws + n.o_vf + m * 2 * in : nullptr,
                 nullptr, wv, nw);
      LSM_SYNC();
    }
    if (n.io.dx0)
      for (int i = tid; i < rows * n.in0; i += nt) {
        const int r = i / n.in0, c = i - r * n.in0;
        n.io.dx0[m0 * n.in0 + i] = B1[r * S1 + c];
      }
    if (n.io.dx1)
      for (int i = tid; i < rows * n.in1; i += nt) {
        const int r = i / n.in1, c = i - r * n.in1;
        n.io.dx1[m0 * n.in1 + i] = B1[r * S1 + n.in0 + c];
      }
    LSM_SYNC();
  }
}

// ---- stage 3: the weight gradients --------------------------------------------------------------------------

// thread tid of the workgroup of (slab, tile): its 4 x 4 entries of the tile's job over the slab's rows
LSM_HD void dw_thread(const Bwd& n, int tile, int64_t slab, int tid) {
  int q = 0;
  while (q + 1 < n.njobs && tile >= n.job[q + 1].tile0) ++q;
  const Job& jb = n.job[q];
  const int t = tile - jb.tile0;
  const int nout = jb.nout, nin = jb.nin;
  const int j = (t / jb.ti_n) * DW_TILE + 4 * (tid / 16);
  const int i = (t % jb.ti_n) * DW_TILE + 4 * (tid % 16);
  if (j >= nout || i > nin) return;
  const float* ws = static_cast<const float*>(n.io.workspace);
  const float* __restrict__ d = ws + jb.d;
  const float* __restrict__ x = ws + jb.x;
  float* part = static_cast<float*>(n.io.workspace) + n.o_part + slab * n.NW;
  const int64_t mb = slab * SLAB;
  const int64_t me = mb + SLAB < n.R ? mb + SLAB : n.R;
  int ja[4], ia[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    ja[a] = j + a < nout ? j + a : nout - 1;
    ia[a] = i + a < nin ? i + a : -1;   // -1: the bias column (i + a == nin), or past it and dropped
  }
  // rows ascending in three levels, all float32: an FMA chain over DW_RUN rows, the runs added in turn into
  // the sum of DW_RUN runs, those added in turn into the slab's: the rounding grows with the levels' lengths
  // (16, 16, 8), not with the slab's 2048
  // The bias column (a plain column sum, whose terms may cancel to far below their size) is summed with the
  // rounding of every addition kept (Knuth's two-sum, rows ascending, float32) and added back at the end.
  float acc[4][4], mid[4][4], run[4][4];
  float bs[4] = {0.0f, 0.0f, 0.0f, 0.0f}, be[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const bool has_bias = i + 4 > nin;   // i <= nin holds here
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = mid[a][b] = 0.0f;
  for (int64_t m1 = mb; m1 < me; m1 += DW_RUN * DW_RUN) {
    const int64_t e1 = m1 + DW_RUN * DW_RUN < me ? m1 + DW_RUN * DW_RUN : me;
    for (int64_t m2 = m1; m2 < e1; m2 += DW_RUN) {
      const int64_t e2 = m2 + DW_RUN < e1 ? m2 + DW_RUN : e1;
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) run[a][b] = 0.0f;
      for (int64_t m = m2; m < e2; ++m) {
        float dv[4], xv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          dv[a] = d[m * nout + ja[a]];
          xv[a] = ia[a] >= 0 ? x[m * nin + ia[a]] : 1.0f;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) run[a][b] = fma_(dv[a], xv[b], run[a][b]);
        if (has_bias) {
#pragma unroll
          for (int a = 0; a < 4; ++a) {
            const float s = bs[a] + dv[a];
            const float bb = s - bs[a];
            be[a] += (bs[a] - (s - bb)) + (dv[a] - bb);
            bs[a] = s;
          }
        }
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) mid[a][b] += run[a][b];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] += mid[a][b], mid[a][b] = 0.0f;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    if (j + a >= nout) continue;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      if (i + b < nin)
        part[jb.w + (int64_t)(j + a) * nin + i + b] = acc[a][b];
      else if (i + b == nin)
        part[jb.b + j + a] = bs[a] + be[a];
    }
  }
}

// entry e of dweights: the slabs' partials in ascending order in float64, rounded once
LSM_HD void finish_entry(const Bwd& n, int64_t e) {
  if (!n.fnorm && e < 2 * (int64_t)n.in) {
    n.io.dweights[e] = 0.0f;
    return;
  }
  const float* part = static_cast<const float*>(n.io.workspace) + n.o_part;
  double s = 0.0;
  for (int64_t k = 0; k < n.slabs; ++k) s += (double)part[k * n.NW + e];
  n.io.dweights[e] = (float)s;
}

__global__ __launch_bounds__(BLOCK) void fwd_kernel(Bwd n, const float* __restrict__ w) {
  const Tile t = block_tile(n.C);
  fwd_tile(n, w, t.row0, t.rows, t.lane, t.wv, WAVES, TILE, t.lds);
}

__global__ __launch_bounds__(BLOCK) void bwd_kernel(Bwd n, const float* __restrict__ w) {
  const Tile t = block_tile(n.C);
  bwd_tile(n, w, t.row0, t.rows, t.lane, t.wv, WAVES, TILE, t.lds);
}

__global__ __launch_bounds__(BLOCK) void dw_kernel(Bwd n) {
  dw_thread(n, (int)blockIdx.y, (int64_t)blockIdx.x, (int)threadIdx.x);
}

__global__ __launch_bounds__(BLOCK) void finish_kernel(Bwd n) {
  const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e < n.NW) finish_entry(n, e);
}

int fail(const char* msg) { return refuse("backward: ", msg); }

size_t fwd_tile_floats(const Bwd& n) { return (size_t)n.SX + 2 * (size_t)n.SA + (size_t)n.RN * n.SH; }
size_t bwd_tile_floats(const Bwd& n) { return (size_t)n.S0 + n.S1 + n.S2 + (size_t)n.RN * n.SH; }

// the config's and the sizes' part of a call: the LDS strides, the workspace layout and the jobs; 0 when fine
int make_plan(const lsm_head_config& c, int64_t C, int32_t T, Bwd* n) {
  const size_t nw = layout(c, n, "backward: ");
  if (nw == 0) return 1;
  if (check_sizes("backward: ", "C", "T * C", "minibatch", C, T)) return 1;
  const int Hd = n->Hd, in = n->in, A = n->A, L = n->L, RN = n->RN;
  n->NW = (int64_t)nw;
  n->C = C;
  n->T = T;
  n->R = C * T;
  n->slabs = (n->R + SLAB - 1) / SLAB;
  n->SA = pad(Hd);   // stage 1 has no logits row
  n->SH = pad(Hd);
  n->HP = (Hd + 3) & ~3;
  const int g = RN > 0 ? 4 * n->HP : Hd;
  n->S0 = pad(in > g ? in : g);
  n->S1 = pad(in > Hd ? (in > A ? in : A) : (Hd > A ? Hd : A));
  n->S2 = pad(Hd);
  const size_t need1 = tile_bytes(fwd_tile_floats(*n)), need2 = tile_bytes(bwd_tile_floats(*n));
  if (need1 > (size_t)WORKGROUP_LDS_BYTES || need2 > (size_t)WORKGROUP_LDS_BYTES) {
    char msg[240];
    snprintf(msg, sizeof msg,
             "the 64-chunk tile needs %zu bytes of LDS in the forward stage and %zu in the backward sweep (rows of "
             "%d, %d, %d and %d x %d floats), a workgroup has %d: use a smaller hidden or recurrent_N, or narrower "
             "inputs",
             need1, need2, n->S0, n->S1, n->S2, RN, n->SH, WORKGROUP_LDS_BYTES);
    return fail(msg);
  }
  // the workspace: [R][width] arrays, then the slabs' partial blobs
  int64_t o = 0;
  const int64_t R = n->R;
  auto take = [&o, R](int width) {
    const int64_t at = o;
    o += R * width;
    return at;
  };
  n->o_u0 = take(in);
  for (int k = 0; k <= MAX_LAYERS; ++k) n->o_p[k] = n->o_y[k] = n->o_v[k] = n->o_dl[k] = 0;
  for (int k = 0; k < MAX_RNN; ++k)
    n->o_hm[k] = n->o_r[k] = n->o_z[k] = n->o_g[k] = n->o_hg[k] = n->o_ho[k] = n->o_di[k] = n->o_dh[k] = 0;
  for (int k = 0; k <= L; ++k) n->o_p[k] = take(Hd), n->o_y[k] = take(Hd);
  for (int k = 0; k < RN; ++k) {
    n->o_hm[k] = take(Hd), n->o_r[k] = take(Hd), n->o_z[k] = take(Hd);
    n->o_g[k] = take(Hd), n->o_hg[k] = take(Hd), n->o_ho[k] = take(Hd);
  }
  n->o_feat = take(Hd);
  n->o_dout = take(A);
  n->o_vr = RN > 0 ? take(2 * Hd) : 0;
  for (int k = 0; k < RN; ++k) n->o_di[k] = take(3 * Hd), n->o_dh[k] = take(3 * Hd);
  for (int k = 0; k <= L; ++k) n->o_v[k] = take(2 * Hd), n->o_dl[k] = take(Hd);
  n->o_vf = n->fnorm ? take(2 * in) : 0;
  n->o_part = o;
  o += n->slabs * n->NW;
  n->ws_floats = o;
  // the jobs, in the blob's order
  int q = 0, tiles = 0;
  int64_t covered = n->fnorm ? 0 : 2 * in;
  auto add = [&](int64_t d, int nout, int64_t x, int nin, int w_off, int b_off) {
    Job& jb = n->job[q++];
    jb.d = d, jb.x = x, jb.nout = nout, jb.nin = nin, jb.w = w_off, jb.b = b_off;
    jb.tile0 = tiles;
    jb.ti_n = (nin + 1 + DW_TILE - 1) / DW_TILE;
    tiles += jb.ti_n * ((nout + DW_TILE - 1) / DW_TILE);
    covered += (int64_t)nout * (nin + 1);
  };
  if (n->fnorm) add(n->o_vf, 2 * in, 0, 0, 0, n->o_fn);
  for (int k = 0; k <= L; ++k) {
    const int din = k == 0 ? in : Hd;
    add(n->o_dl[k], Hd, k == 0 ? n->o_u0 : n->o_y[k - 1], din, n->o_fc[k], n->o_fc[k] + Hd * din);
    add(n->o_v[k], 2 * Hd, 0, 0, 0, n->o_fc[k] + Hd * din + Hd);
  }
  for (int k = 0; k < RN; ++k) {
    const int g0 = n->o_gru[k];
    add(n->o_di[k], 3 * Hd, k == 0 ? n->o_y[L] : n->o_ho[k - 1], Hd, g0, g0 + 6 * Hd * Hd);
    add(n->o_dh[k], 3 * Hd, n->o_hm[k], Hd, g0 + 3 * Hd * Hd, g0 + 6 * Hd * Hd + 3 * Hd);
  }
  if (RN > 0) add(n->o_vr, 2 * Hd, 0, 0, 0, n->o_rn);
  add(n->o_dout, A, n->o_feat, Hd, n->o_out, n->o_out + A * Hd);
  n->njobs = q;
  n->ntiles = tiles;
  if (covered != n->NW) return fail("internal: the jobs do not cover the blob");
  return 0;
}

// every check of one call, shared by the device and the host entry point; fills n; 0 when fine
int make_bwd(const lsm_head_config& c, const float* weights, const lsm_bwd_io* io, int64_t C, int32_t T, Bwd* n) {
  if (make_plan(c, C, T, n)) return 1;
  if (!weights) return fail("weights is null");
  if (!io) return fail("io is null");
  lsm_bwd_io f = *io;
  const bool actor = n->kind == LSM_HEAD_ACTOR;
  drop_unread(*n, &f);
  if (n->in0 == 0) f.dx0 = nullptr;
  if (n->in1 == 0) f.dx1 = nullptr;
  if (actor)
    f.dvalues = nullptr;
  else
    f.dlogits = f.available_actions = nullptr;
  if (!f.dweights) return fail("dweights is null");
  if (!f.workspace) return fail("workspace is null");
  if (const char* why = inputs_missing(*n, f, C)) return fail(why);
  if (const char* why = states_missing(*n, f, C)) return fail(why);
  if (C > 0 && actor && !f.dlogits) return fail("the actor needs dlogits");
  if (C > 0 && !actor && !f.dvalues) return fail("the critic needs dvalues");
  if (const char* why = misaligned({weights, f.x0, f.x1, f.rnn_states, f.masks, f.available_actions, f.dlogits,
                                    f.dvalues, f.dweights, f.dx0, f.dx1}))
    return fail(why);
  if (const char* why = misaligned({f.workspace}, 7, "misaligned pointer (workspace: 8 bytes)")) return fail(why);
  const size_t F = sizeof(float), R = (size_t)n->R;
  struct Range {
    const void* p;
    size_t bytes;
  };
  const Range outs[] = {{f.dweights, (size_t)n->NW * F},
                        {f.dx0, R * n->in0 * F},
                        {f.dx1, R * n->in1 * F},
                        {f.workspace, (size_t)n->ws_floats * F}};
  const Range ins[] = {{weights, (size_t)n->NW * F},
                       {f.x0, R * n->in0 * F},
                       {f.x1, R * n->in1 * F},
                       {f.rnn_states, (size_t)C * n->RN * n->Hd * F},
                       {f.masks, R * F},
                       {f.available_actions, R * n->A * F},
                       {f.dlogits, R * n->A * F},
                       {f.dvalues, R * F}};
  for (int a = 0; a < 4; ++a) {
    for (const Range& b : ins)
      if (overlap(outs[a].p, outs[a].bytes, b.p, b.bytes)) return fail("an output overlaps an input");
    for (int b = a + 1; b < 4; ++b)
      if (overlap(outs[a].p, outs[a].bytes, outs[b].p, outs[b].bytes)) return fail("two outputs overlap");
  }
  n->w = weights;
  n->io = f;
  return 0;
}

}  // namespace

int lsm_backward_fill_plan(const lsm_head_config& c, int64_t C, int32_t T, lsm_head_launch_plan* out) {
  Bwd n;
  if (make_plan(c, C, T, &n)) return 1;
  static_assert(MAX_JOBS == LSM_HEAD_PLAN_MAX_JOBS, "lsm_policy.h's job array holds every job");
  out->SX = n.SX, out->SA = n.SA, out->SH = n.SH;
  out->S0 = n.S0, out->S1 = n.S1, out->S2 = n.S2, out->HP = n.HP;
  out->njobs = n.njobs, out->ntiles = n.ntiles;
  out->lds_bytes[0] = (int64_t)tile_bytes(fwd_tile_floats(n));
  out->lds_bytes[1] = (int64_t)tile_bytes(bwd_tile_floats(n));
  out->slabs = n.slabs;
  out->ws_floats = n.ws_floats;
  out->o_feat = n.o_feat;
  for (int k = 0; k < MAX_RNN; ++k) out->o_ho[k] = n.o_ho[k];
  for (int q = 0; q < n.njobs; ++q) {
    const Job& jb = n.job[q];
    out->job[q].nout = jb.nout, out->job[q].nin = jb.nin, out->job[q].ti_n = jb.ti_n, out->job[q].tile0 = jb.tile0;
  }
  return 0;
}

extern "C" {

size_t lsm_head_backward_workspace_bytes(lsm_head_config cfg, int64_t C, int32_t T) {
  Bwd n;
  if (make_plan(cfg, C, T, &n)) return 0;
  const size_t bytes = ((size_t)n.ws_floats * sizeof(float) + 7) & ~(size_t)7;
  return bytes < 8 ? 8 : bytes;
}

int lsm_head_backward(lsm_head_config cfg, const float* weights, const lsm_bwd_io* io, int64_t C, int32_t T,
                      void* hip_stream) {
  Bwd n;
  if (make_bwd(cfg, weights, io, C, T, &n)) return 1;
  if (C == 0) return 0;
  const dim3 grid((unsigned)tiles_of(C));
  const size_t lds1 = tile_bytes(fwd_tile_floats(n)), lds2 = tile_bytes(bwd_tile_floats(n));
  // the LDS limits: to a workgroup's whole LDS
  const char* why = raise_lds<fwd_kernel, WORKGROUP_LDS_BYTES>();
  if (!why) why = raise_lds<bwd_kernel, WORKGROUP_LDS_BYTES>();
  if (!why) why = launch<fwd_kernel, WORKGROUP_LDS_BYTES>(grid, BLOCK, lds1, hip_stream, n, n.w);
  if (!why) why = launch<bwd_kernel, WORKGROUP_LDS_BYTES>(grid, BLOCK, lds2, hip_stream, n, n.w);
  if (!why) why = launch<dw_kernel>(dim3((unsigned)n.slabs, (unsigned)n.ntiles), BLOCK, 0, hip_stream, n);
  if (!why) why = launch<finish_kernel>((unsigned)((n.NW + BLOCK - 1) / BLOCK), BLOCK, 0, hip_stream, n);
  return why ? fail(why) : 0;
}

int lsm_host_head_backward(lsm_head_config cfg, const float* weights, const lsm_bwd_io* io, int64_t C, int32_t T) {
  Bwd n;
  if (make_bwd(cfg, weights, io, C, T, &n)) return 1;
  if (C == 0) return 0;
  const size_t f1 = fwd_tile_floats(n), f2 = bwd_tile_floats(n);
  std::vector<float4> lds((f1 > f2 ? f1 : f2) / 4 + 1);
  for (int64_t b = 0; b < C; ++b) fwd_tile(n, n.w, b, 1, 0, 0, 1, 1, reinterpret_cast<float*>(lds.data()));
  for (int64_t b = 0; b < C; ++b) bwd_tile(n, n.w, b, 1, 0, 0, 1, 1, reinterpret_cast<float*>(lds.data()));
  for (int64_t s = 0; s < n.slabs; ++s)
    for (int t = 0; t < n.ntiles; ++t)
      for (int tid = 0; tid < BLOCK; ++tid) dw_thread(n, t, s, tid);
  for (int64_t e = 0; e < n.NW; ++e) finish_entry(n, e);
  return 0;
}

}  // extern "C"
