// Actor-critic heads, Categorical distribution and the PPO loss (K13-K15).
//
// Reference:
//   critic_linear / Categorical.linear  model.py:182-199, distributions.py:54-68
//   FixedCategorical sample / log_probs / mode / entropy  distributions.py:17-27
//     (torch Categorical: logits -= logsumexp; probs = softmax(logits);
//      sample = multinomial(probs,1) = argmax(probs / E), E ~ Exp(1);
//      entropy = -Σ logits*probs)
//   Policy.act / evaluate_actions  model.py:54-79
//   PPO clipped surrogate + clipped value loss + entropy  algo/ppo.py:61-81
//
// One wave owns one row at a time.  Lane l holds hidden features
// j = l + 64c (c < HC, H = 64·HC); the head weights for those columns stay in
// registers for all rows the wave processes.  The 1+A head dot products are
// wave-reduced with xor shuffles, so every lane holds value and logits and the
// softmax/sampling/loss arithmetic is computed redundantly (no LDS traffic).
//
// The training kernel is the fused forward + backward of everything above the
// fc layer: loss terms, dL/dlogits and dL/dvalue (analytic, with autograd's
// tie conventions), dL/dfeature masked by the fc ReLU, and per-block partial
// sums of the head weight/bias gradients (deterministic reduce afterwards).
#include "heads_dispatch.h"   // and through it heads_common.h: HW, HeadW, load_head_w, head_dots, act_grad, ...

namespace {

// torch Categorical(logits=z): nl = z - logsumexp(z); p = softmax(nl)
template <int AMAX>
__device__ __forceinline__ void categorical(const float (&z)[AMAX], int A, float (&nl)[AMAX], float (&p)[AMAX]) {
  float mx = z[0];
#pragma unroll
  for (int o = 1; o < AMAX; ++o)
    if (o < A) mx = fmaxf(mx, z[o]);
  float se = 0.f;
#pragma unroll
  for (int o = 0; o < AMAX; ++o)
    if (o < A) se += expf(z[o] - mx);
  const float lse = mx + logf(se);
  float m2 = -INFINITY;
#pragma unroll
  for (int o = 0; o < AMAX; ++o) {
    nl[o] = o < A ? z[o] - lse : -INFINITY;
    if (o < A) m2 = fmaxf(m2, nl[o]);
  }
  float s2 = 0.f;
#pragma unroll
  for (int o = 0; o < AMAX; ++o) {
    p[o] = o < A ? expf(nl[o] - m2) : 0.f;
    s2 += p[o];
  }
#pragma unroll
  for (int o = 0; o < AMAX; ++o) p[o] = p[o] / s2;
}

// A stored / given action as an index: the range is decided on the 64-bit value
// (2^32 + 2 must not pass as 2); anything outside [0, A) becomes -1, which no
// later `(unsigned)act < (unsigned)A` or `o == act` accepts.
__device__ __forceinline__ int action_index(int64_t v, int A) {
  return (uint64_t)v < (uint64_t)A ? (int)v : -1;
}

__device__ __forceinline__ float exp_noise(uint64_t seed, uint64_t counter, long long row, int o, int A) {
  const uint64_t h = mix64(seed ^ mix64(counter * 0x2545F4914F6CDD1Dull + (uint64_t)(row * A + o)));
  return -logf(u01_open0(h));
}

// act / evaluate: value, action (sample | mode | given), log_prob, entropy
// FAST: A == AMAX, H == 64·HC, no separate critic features (compile-time bounds)
template <int HC, int AMAX, bool FAST>
__global__ __launch_bounds__(64 * HW) void heads_act_kernel(
    const float* __restrict__ feat, const float* __restrict__ feat_v_, int N, int H_, const float* __restrict__ wc,
    const float* __restrict__ bc, const float* __restrict__ wa, const float* __restrict__ ba, int A_,
    const float* __restrict__ noise,
    unsigned long long seed, unsigned long long counter_v, const unsigned long long* __restrict__ counter_p,
    int deterministic, const int64_t* __restrict__ given,
    float* __restrict__ value_out, int64_t* __restrict__ action_out, float* __restrict__ logp_out,
    float* __restrict__ ent_out, int rows_per_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = FAST ? 64 * HC : H_, A = FAST ? AMAX : A_;
  const float* const feat_v = FAST ? nullptr : feat_v_;
  const uint64_t counter = rng_counter_of(counter_p, counter_v);
  HeadW<HC, AMAX> w;
  load_head_w(w, wc, wa, A, H, lane);
  const float b0 = bc[0];
  const long long r0 = ((long long)blockIdx.x * HW + wave) * rows_per_wave;
  for (int rr = 0; rr < rows_per_wave; ++rr) {
    const long long row = r0 + rr;
    if (row >= N) break;
    float f[HC], fv[HC];
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      const bool in = lane + 64 * c < H;
      f[c] = in ? feat[row * H + lane + 64 * c] : 0.f;
      fv[c] = feat_v ? (in ? feat_v[row * H + lane + 64 * c] : 0.f) : f[c];
    }
    float value, z[AMAX], nl[AMAX], p[AMAX];
    head_dots(w, f, fv, value, z, b0, ba, A);
    categorical(z, A, nl, p);
    int act;
    if (given) {
      act = action_index(given[row], A);
    } else {
      act = 0;
      float best = -INFINITY;
#pragma unroll
      for (int o = 0; o < AMAX; ++o) {
        if (o < A) {
          const float sc = deterministic ? p[o] : p[o] / (noise ? noise[row * A + o] : exp_noise(seed, counter, row, o, A));
          if (sc > best) { best = sc; act = o; }
        }
      }
    }
    // an action index outside [0, A) has no log-prob: the reference's gather
    // raises there (distributions.py:22); NaN marks the row here
    float lp = (unsigned)act < (unsigned)A ? 0.f : __int_as_float(0x7fc00000), ent = 0.f;
#pragma unroll
    for (int o = 0; o < AMAX; ++o) {
      if (o == act && o < A) lp = nl[o];
      if (o < A) ent -= nl[o] * p[o];
    }
    if (lane == 0) {
      if (value_out) value_out[row] = value;
      if (action_out) action_out[row] = act;
      if (logp_out) logp_out[row] = lp;
      if (ent_out) ent_out[row] = ent;
    }
  }
}

struct TrainArgs {
  const float* feat;  // [B][H] policy features (CNNBase: post-ReLU fc; MLPBase: actor tanh output)
  const float* feat_v;  // [B][H] critic features (MLPBase) or NULL (= feat)
  int B, H, A;
  const float *wc, *bc, *wa, *ba;
  const int64_t* idx;      // storage row of each sample (nullable: row0 + b)
  long long row0;
  const int64_t* actions;  // storage planes, indexed by storage row
  const float *old_logp, *adv, *vpred, *ret;   // LOSS_A2C reads only ret; the other three may be NULL
  float clip, value_coef, entropy_coef, inv_b;
  int use_clipped_value_loss;
  int loss_kind;           // LOSS_PPO | LOSS_A2C (heads_common.h)
  int feat_act;            // activation producing the features: 0 none (GRU), 1 ReLU, 2 tanh
  float* dfeat;            // [B][H] dL/d(feature pre-activation) (both heads when dfeat_v is NULL)
  float* dfeat_v;          // [B][H] critic-branch gradient (MLPBase) or NULL
  float* part_w;           // [blocks][1+A][H]
  float* part_b;           // [blocks][1+A]
  float* part_loss;        // [blocks][4]: Σ max(l1,l2), Σ min(s1,s2), Σ H, # actions outside [0, A)
  int rows_per_wave;
};

// FAST: A == AMAX, H == 64·HC, no separate critic features / gradient (CNNBase
// and the GRU policy): every per-lane and per-action bound is a compile-time
// constant, which removes the uniform branches around each unrolled operation
// (the generic instantiation runs ~2,500 instructions per row).
// LK: LOSS_RT, or the loss kind fixed at compile time (split_loss, heads_common.h).
template <int HC, int AMAX, bool FAST, int LK>
__global__ __launch_bounds__(64 * HW) void heads_train_kernel(const TrainArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int loss_kind = loss_kind_of<LK>(a.loss_kind);
  const int H = FAST ? 64 * HC : a.H, A = FAST ? AMAX : a.A;
  const float* const feat_v = FAST ? nullptr : a.feat_v;
  float* const dfeat_v = FAST ? nullptr : a.dfeat_v;
  HeadW<HC, AMAX> w;
  load_head_w(w, a.wc, a.wa, A, H, lane);
  const float b0 = a.bc[0];
  float gwc[HC], gwa[AMAX][HC], gbc = 0.f, gba[AMAX];
#pragma unroll
  for (int c = 0; c < HC; ++c) gwc[c] = 0.f;
#pragma unroll
  for (int o = 0; o < AMAX; ++o) {
    gba[o] = 0.f;
#pragma unroll
    for (int c = 0; c < HC; ++c) gwa[o][c] = 0.f;
  }
  float s_vl = 0.f, s_al = 0.f, s_ent = 0.f, s_bad = 0.f;
  const long long r0 = ((long long)blockIdx.x * HW + wave) * a.rows_per_wave;
  // The per-row storage scalars (the minibatch gather idx -> action, advantage,
  // old log-prob, value, return) of all of this wave's rows are fetched up
  // front, lane j holding row r0 + j (rows_per_wave <= 64), and broadcast with
  // readlane per row; each row's features are loaded one row ahead.  Without
  // this the wave waited on two dependent loads per row (latency-bound).
  int q_act = 0;
  float q_adv = 0.f, q_olp = 0.f, q_vo = 0.f, q_ret = 0.f;
  if (lane < a.rows_per_wave && r0 + lane < a.B) {
    const long long sr = a.idx ? (long long)a.idx[r0 + lane] : a.row0 + r0 + lane;
    q_act = action_index(a.actions[sr], A);
    if (loss_kind != LOSS_A2C) {   // A2C: the three pointers may be NULL
      q_adv = a.adv[sr];
      q_olp = a.old_logp[sr];
      q_vo = a.vpred[sr];
    }
    q_ret = a.ret[sr];
  }
  float fn[HC], fvn[HC];
  auto load_row = [&](long long row) {
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      const bool in = row < a.B && lane + 64 * c < H;
      fn[c] = in ? a.feat[row * H + lane + 64 * c] : 0.f;
      fvn[c] = feat_v ? (in ? feat_v[row * H + lane + 64 * c] : 0.f) : fn[c];
    }
  };
  load_row(r0);
  for (int rr = 0; rr < a.rows_per_wave; ++rr) {
    const long long row = r0 + rr;
    if (row >= a.B) break;
    float f[HC], fv[HC];
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      f[c] = fn[c];
      fv[c] = fvn[c];
    }
    if (rr + 1 < a.rows_per_wave) load_row(row + 1);
    float value, z[AMAX], nl[AMAX], p[AMAX];
    head_dots(w, f, fv, value, z, b0, a.ba, A);
    categorical(z, A, nl, p);
    const int act = __builtin_amdgcn_readlane(q_act, rr);
    s_bad += (unsigned)act < (unsigned)A ? 0.f : 1.f;   // counted; PPO.update raises (gather's IndexError)
    float lp = 0.f, ent = 0.f;
#pragma unroll
    for (int o = 0; o < AMAX; ++o) {
      if (o == act) lp = nl[o];
      if (o < A) ent -= nl[o] * p[o];
    }
    const float R = bcast(q_ret, rr);
    float g_logp, g_v;
    if (loss_kind == LOSS_A2C) {
      a2c_row_loss(value, lp, R, a.value_coef, a.inv_b, g_logp, g_v, s_vl, s_al);   // a2c_acktr.py:48-51
    } else {
      ppo_row_loss(a, value, lp, LaneOf{q_adv, rr}, LaneOf{q_olp, rr}, LaneOf{q_vo, rr}, R, g_logp, g_v, s_vl,
                   s_al);   // ppo.py:61-77
    }
    s_ent += ent;
    // dL/dlogits = g_logp (onehot - p) + (c_e/B) p (nl + H)
    float gz[AMAX];
    const float ce = a.entropy_coef * a.inv_b;
#pragma unroll
    for (int o = 0; o < AMAX; ++o)
      gz[o] = o < A ? g_logp * ((o == act ? 1.f : 0.f) - p[o]) + ce * p[o] * (nl[o] + ent) : 0.f;
    // dL/dh for this lane's columns, masked by the fc ReLU; head grads
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      const float dv = g_v * w.wc[c];
      float d = dfeat_v ? 0.f : dv;
#pragma unroll
      for (int o = 0; o < AMAX; ++o) d += gz[o] * w.wa[o][c];
      if (lane + 64 * c < H) {
        const size_t q = (size_t)row * H + lane + 64 * c;
        a.dfeat[q] = act_grad(d, f[c], a.feat_act);
        if (dfeat_v) dfeat_v[q] = act_grad(dv, fv[c], a.feat_act);
      }
      gwc[c] += g_v * fv[c];
#pragma unroll
      for (int o = 0; o < AMAX; ++o) gwa[o][c] += gz[o] * f[c];
    }
    gbc += g_v;
#pragma unroll
    for (int o = 0; o < AMAX; ++o) gba[o] += gz[o];
  }
  // block reduction of the head-gradient partials across the HW waves
  __shared__ float red[HW][64 * HC];
  __shared__ float redb[HW][AMAX + 5];
  const int NO = 1 + A;
  for (int o = 0; o < NO; ++o) {
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      float v = gwc[c];
#pragma unroll
      for (int q = 0; q < AMAX; ++q)
        if (o == q + 1) v = gwa[q][c];
      red[wave][lane + 64 * c] = v;
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int c = 0; c < HC; ++c) {
        const int j = lane + 64 * c;
        float s = red[0][j];
        for (int q = 1; q < HW; ++q) s += red[q][j];
        if (j < H) a.part_w[((size_t)blockIdx.x * NO + o) * H + j] = s;
      }
    }
    __syncthreads();
  }
  if (lane == 0) {
    redb[wave][0] = gbc;
#pragma unroll
    for (int o = 0; o < AMAX; ++o) redb[wave][1 + o] = gba[o];
    redb[wave][AMAX + 1] = s_vl;
    redb[wave][AMAX + 2] = s_al;
    redb[wave][AMAX + 3] = s_ent;
    redb[wave][AMAX + 4] = s_bad;
  }
  __syncthreads();
  if (threadIdx.x < NO) {
    float s = 0.f;
    for (int q = 0; q < HW; ++q) s += redb[q][threadIdx.x];
    a.part_b[(size_t)blockIdx.x * NO + threadIdx.x] = s;
  }
  if (threadIdx.x < 4) {
    float s = 0.f;
    for (int q = 0; q < HW; ++q) s += redb[q][AMAX + 1 + threadIdx.x];
    a.part_loss[(size_t)blockIdx.x * 4 + threadIdx.x] = s;
  }
}

// heads_train_kernel for CNNBase / the GRU policy at H = 512, A = 8 (TrainArgs'
// FAST case) with the head weights in LDS instead of registers: a lane holds the
// columns 4·lane + q + 256·c2 (q < 4, c2 < 2: float4 loads and stores of the
// features and their gradient) and reads the 9 weight rows of those columns as
// 18 ds_read_b128 per row pass.  The register version held 72 weight VGPRs next
// to the 72 gradient accumulators (256 VGPRs: one wave per SIMD, every row's
// dependent chain — 9 wave reductions, the softmax, the loss — exposed); this one
// fits two waves per SIMD.  Same arithmetic per element, same partial layout.
__global__ __launch_bounds__(64 * HW) void heads_train_lds_kernel(const TrainArgs a) {
  constexpr int A = 8, H = 512;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ f32x4 Wl[9][128];   // row 0: critic, rows 1..8: actor logits (the flat parameter
  for (int i = threadIdx.x; i < 9 * H; i += 64 * HW) {   // buffer places wa at an odd offset: scalar loads)
    const int o = i / H, k = i - H * o;
    reinterpret_cast<float*>(&Wl[o][0])[k] = o == 0 ? a.wc[k] : a.wa[(o - 1) * H + k];
  }
  const float b0 = a.bc[0];
  float ba[A];
#pragma unroll
  for (int o = 0; o < A; ++o) ba[o] = a.ba[o];
  __syncthreads();
  f32x4 gw[9][2];   // Σ_rows g_o · f (o = 0: critic), this lane's columns
#pragma unroll
  for (int o = 0; o < 9; ++o) gw[o][0] = gw[o][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  float gbc = 0.f, gba[A];
#pragma unroll
  for (int o = 0; o < A; ++o) gba[o] = 0.f;
  float s_vl = 0.f, s_al = 0.f, s_ent = 0.f, s_bad = 0.f;
  const long long r0 = ((long long)blockIdx.x * HW + wave) * a.rows_per_wave;
  int q_act = 0;
  float q_adv = 0.f, q_olp = 0.f, q_vo = 0.f, q_ret = 0.f;
  if (lane < a.rows_per_wave && r0 + lane < a.B) {
    const long long sr = a.idx ? (long long)a.idx[r0 + lane] : a.row0 + r0 + lane;
    q_act = action_index(a.actions[sr], A);
    if (a.loss_kind != LOSS_A2C) {   // A2C: the three pointers may be NULL
      q_adv = a.adv[sr];
      q_olp = a.old_logp[sr];
      q_vo = a.vpred[sr];
    }
    q_ret = a.ret[sr];
  }
  f32x4 fn[2];
  auto load_row = [&](long long row) {
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
      fn[c2] = row < a.B ? reinterpret_cast<const f32x4*>(a.feat + row * H)[lane + 64 * c2] : f32x4{0.f, 0.f, 0.f, 0.f};
  };
  load_row(r0);
  for (int rr = 0; rr < a.rows_per_wave; ++rr) {
    const long long row = r0 + rr;
    if (row >= a.B) break;
    const f32x4 f[2] = {fn[0], fn[1]};
    if (rr + 1 < a.rows_per_wave) load_row(row + 1);
    float dots[9];
#pragma unroll
    for (int o = 0; o < 9; ++o) {
      float t = 0.f;
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        const f32x4 w = Wl[o][lane + 64 * c2];
#pragma unroll
        for (int q = 0; q < 4; ++q) t += f[c2][q] * w[q];
      }
      dots[o] = wave_sum(t);
    }
    const float value = dots[0] + b0;
    float z[A], nl[A], p[A];
#pragma unroll
    for (int o = 0; o < A; ++o) z[o] = dots[1 + o] + ba[o];
    categorical(z, A, nl, p);
    const int act = __builtin_amdgcn_readlane(q_act, rr);
    s_bad += (unsigned)act < (unsigned)A ? 0.f : 1.f;
    float lp = 0.f, ent = 0.f;
#pragma unroll
    for (int o = 0; o < A; ++o) {
      if (o == act) lp = nl[o];
      ent -= nl[o] * p[o];
    }
    const float R = bcast(q_ret, rr);
    float g_logp, g_v;
    if (a.loss_kind == LOSS_A2C) {
      a2c_row_loss(value, lp, R, a.value_coef, a.inv_b, g_logp, g_v, s_vl, s_al);   // a2c_acktr.py:48-51
    } else {
      ppo_row_loss(a, value, lp, LaneOf{q_adv, rr}, LaneOf{q_olp, rr}, LaneOf{q_vo, rr}, R, g_logp, g_v, s_vl,
                   s_al);   // ppo.py:61-77
    }
    s_ent += ent;
    float g[9];   // g[0] = dL/dvalue, g[1 + o] = dL/dlogit o
    g[0] = g_v;
    const float ce = a.entropy_coef * a.inv_b;
#pragma unroll
    for (int o = 0; o < A; ++o) g[1 + o] = g_logp * ((o == act ? 1.f : 0.f) - p[o]) + ce * p[o] * (nl[o] + ent);
    // dL/dfeature of this lane's columns (masked by the activation), head gradients
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      f32x4 d = Wl[0][lane + 64 * c2] * g[0];
#pragma unroll
      for (int o = 1; o < 9; ++o) {
        const f32x4 w = Wl[o][lane + 64 * c2];
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] += g[o] * w[q];
      }
      f32x4 y;
#pragma unroll
      for (int q = 0; q < 4; ++q) y[q] = act_grad(d[q], f[c2][q], a.feat_act);
      reinterpret_cast<f32x4*>(a.dfeat + row * H)[lane + 64 * c2] = y;
#pragma unroll
      for (int o = 0; o < 9; ++o)
#pragma unroll
        for (int q = 0; q < 4; ++q) gw[o][c2][q] += g[o] * f[c2][q];
    }
    gbc += g_v;
#pragma unroll
    for (int o = 0; o < A; ++o) gba[o] += g[1 + o];
  }
  // block reduction of the head-gradient partials across the HW waves (fixed order)
  __shared__ f32x4 red[HW][128];
  __shared__ float redb[HW][A + 5];
  for (int o = 0; o < 9; ++o) {
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) red[wave][lane + 64 * c2] = gw[o][c2];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        f32x4 t = red[0][lane + 64 * c2];
        for (int q = 1; q < HW; ++q) t += red[q][lane + 64 * c2];
        reinterpret_cast<f32x4*>(a.part_w + ((size_t)blockIdx.x * 9 + o) * H)[lane + 64 * c2] = t;
      }
    }
    __syncthreads();
  }
  if (lane == 0) {
    redb[wave][0] = gbc;
#pragma unroll
    for (int o = 0; o < A; ++o) redb[wave][1 + o] = gba[o];
    redb[wave][A + 1] = s_vl;
    redb[wave][A + 2] = s_al;
    redb[wave][A + 3] = s_ent;
    redb[wave][A + 4] = s_bad;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    float t = 0.f;
    for (int q = 0; q < HW; ++q) t += redb[q][threadIdx.x];
    a.part_b[(size_t)blockIdx.x * 9 + threadIdx.x] = t;
  }
  if (threadIdx.x < 4) {
    float t = 0.f;
    for (int q = 0; q < HW; ++q) t += redb[q][A + 1 + threadIdx.x];
    a.part_loss[(size_t)blockIdx.x * 4 + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(256) void mean_kernel(const float* __restrict__ x, long long n, float* __restrict__ out) {
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) s += (double)x[i];
  __shared__ double r[256];
  r[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) r[threadIdx.x] += r[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(r[0] / (double)n);
}

// *counter += by, after the act kernel that read it (stream order): an increment inside
// that kernel would race with the blocks that have not read the word yet
__global__ void rng_advance_kernel(unsigned long long* counter, unsigned long long by) { *counter += by; }

// the arguments of one act launch (counter_p: the sampling counter as a word in device
// memory, read by the kernel; NULL: the by-value counter)
struct ActCall {
  const float *feat, *feat_v;
  int N, H;
  const float *wc, *bc, *wa, *ba;
  int A;
  const float* noise;
  unsigned long long seed, counter;
  const unsigned long long* counter_p;
  int det;
  const int64_t* given;
  float* v;
  int64_t* act;
  float *lp, *ent;
  int rows_per_wave;
};

// what heads_dispatch.h needs to know of this family
struct Cat {
  using Act = ActCall;
  using Train = TrainArgs;
  static constexpr const char* noun = "actions";
  static constexpr const char *act_scope = "heads_act", *train_scope = "heads_train";
  static constexpr const char *act_kernel = "heads_act_kernel", *train_kernel = "heads_train_kernel",
                              *train_lds_kernel = "heads_train_lds_kernel";
  static double act_row_bytes(const Act&) { return 16.0; }
  static double train_row_bytes(const Train& a) { return a.loss_kind == LOSS_A2C ? 20.0 : 32.0; }
  // built once per loss kind instead of with the run-time branch (heads_common.h, LOSS_RT):
  // 96 -> 100, 165 -> 169 and 253 -> 257 VGPRs with it
  static constexpr bool split_loss(int HC, int AMAX, bool FAST) {
    return AMAX == 8 && ((HC == 1 && FAST) || (HC == 4 && !FAST) || (HC == 8 && !FAST));
  }
  template <int HC, int AMAX, bool FAST>
  static void launch_act(const Act& c, unsigned blocks, hipStream_t st) {
    heads_act_kernel<HC, AMAX, FAST><<<blocks, 64 * HW, 0, st>>>(c.feat, c.feat_v, c.N, c.H, c.wc, c.bc, c.wa, c.ba, c.A,
                                                         c.noise, c.seed, c.counter, c.counter_p, c.det, c.given, c.v,
                                                         c.act, c.lp, c.ent, c.rows_per_wave);
  }
  template <int HC, int AMAX, bool FAST, int LK>
  static void launch_train(const Train& a, int blocks, hipStream_t st) {
    heads_train_kernel<HC, AMAX, FAST, LK><<<blocks, 64 * HW, 0, st>>>(a);
  }
  static void launch_train_lds(const Train& a, int blocks, hipStream_t st) {
    heads_train_lds_kernel<<<blocks, 64 * HW, 0, st>>>(a);
  }
};

// ppo_heads_act (counter_p NULL) / ppo_heads_act_dc (the counter in device memory)
int cat_act(const char* name, const float* feat, const float* feat_v, int N, int H, const float* wc, const float* bc,
            const float* wa, const float* ba, int A, const float* noise, unsigned long long seed,
            unsigned long long counter, const unsigned long long* counter_p, int deterministic, const int64_t* given,
            float* value, int64_t* action, float* logp, float* entropy, void* stream) {
  const ActCall c = {feat, feat_v, N, H, wc, bc, wa, ba, A, noise, seed, counter, counter_p, deterministic, given,
                     value, action, logp, entropy, /*rows_per_wave*/ 0};
  return heads_act<Cat>(name, c, stream);
}

// ppo_heads_train (LOSS_PPO) / ppo_heads_train_a2c (LOSS_A2C: old_logp, adv and vpred NULL,
// clip and use_clipped_value_loss 0, none of them read)
int cat_train(const char* name, int loss_kind, const float* feat, const float* feat_v, int B, int H, const float* wc,
              const float* bc, const float* wa, const float* ba, int A, const int64_t* idx, long long row0,
              const int64_t* actions, const float* old_logp, const float* adv, const float* vpred, const float* ret,
              float clip, float value_coef, float entropy_coef, float inv_b, int use_clipped_value_loss, int feat_act,
              float* dfeat, float* dfeat_v, float* part_w, float* part_b, float* part_loss, void* stream) {
  const TrainArgs a = {feat, feat_v, B, H, A, wc, bc, wa, ba, idx, row0, actions, old_logp, adv, vpred, ret,
                       clip, value_coef, entropy_coef, inv_b, use_clipped_value_loss, loss_kind, feat_act,
                       dfeat, dfeat_v, part_w, part_b, part_loss, /*rows_per_wave*/ 0};
  return heads_train<Cat>(name, a, stream);
}

}  // namespace

// Policy.act / evaluate_actions heads (model.py:54-79):
//   noise   != NULL: sample = argmax(probs / noise) (host-replay parity mode)
//   noise   == NULL: Exp(1) noise from the counter RNG (seed, counter, row)
//   given   != NULL: log_prob/entropy of the given actions (evaluate_actions)
//   deterministic: mode = argmax(probs)
PPO_API int ppo_heads_act(const float* feat, const float* feat_v, int N, int H, const float* wc, const float* bc,
                          const float* wa,
                          const float* ba, int A, const float* noise, unsigned long long seed,
                          unsigned long long counter, int deterministic, const int64_t* given, float* value,
                          int64_t* action, float* logp, float* entropy, void* stream) {
  return cat_act("ppo_heads_act", feat, feat_v, N, H, wc, bc, wa, ba, A, noise, seed, counter, nullptr, deterministic,
                 given, value, action, logp, entropy, stream);
}

// ppo_heads_act with the counter in device memory: one 8-byte word that the kernel reads
// (once per wave) and never writes, so a launch captured into a HIP graph samples anew at
// every replay once ppo_rng_advance follows it on the stream
PPO_API int ppo_heads_act_dc(const float* feat, const float* feat_v, int N, int H, const float* wc, const float* bc,
                             const float* wa, const float* ba, int A, const float* noise, unsigned long long seed,
                             const unsigned long long* counter, int deterministic, const int64_t* given,
                             float* value, int64_t* action, float* logp, float* entropy, void* stream) {
  PPO_REQUIRE(counter != nullptr, "ppo_heads_act_dc: counter is NULL (a device pointer to one 8-byte word)");
  return cat_act("ppo_heads_act_dc", feat, feat_v, N, H, wc, bc, wa, ba, A, noise, seed, 0ull, counter, deterministic,
                 given, value, action, logp, entropy, stream);
}

// *counter += by (64-bit wrap-around) as a launch of its own on `stream`
PPO_API int ppo_rng_advance(unsigned long long* counter, unsigned long long by, void* stream) {
  PPO_REQUIRE(counter != nullptr, "ppo_rng_advance: counter is NULL (a device pointer to one 8-byte word)");
  rng_advance_kernel<<<1, 1, 0, as_stream(stream)>>>(counter, by);
  PPO_LAUNCH_CHECK("rng_advance_kernel");
  return 0;
}

PPO_API int ppo_heads_train_blocks(int B) {
  const int rpw = 32;
  return (int)ceil_div(B, HW * rpw);
}

PPO_API int ppo_heads_train(const float* feat, const float* feat_v, int B, int H, const float* wc, const float* bc,
                            const float* wa,
                            const float* ba, int A, const int64_t* idx, long long row0, const int64_t* actions,
                            const float* old_logp, const float* adv, const float* vpred, const float* ret, float clip,
                            float value_coef, float entropy_coef, float inv_b, int use_clipped_value_loss,
                            int feat_act, float* dfeat, float* dfeat_v, float* part_w, float* part_b,
                            float* part_loss, void* stream) {
  return cat_train("ppo_heads_train", LOSS_PPO, feat, feat_v, B, H, wc, bc, wa, ba, A, idx, row0, actions, old_logp,
                   adv, vpred, ret, clip, value_coef, entropy_coef, inv_b, use_clipped_value_loss, feat_act, dfeat,
                   dfeat_v, part_w, part_b, part_loss, stream);
}

// ppo_heads_train with A2C's row loss (algo/a2c_acktr.py:48-51, a2c_row_loss): reads only
// the actions and the returns of the storage.  part_loss slot 0 holds Σ 2 (R - v)^2, so
// ppo_heads_reduce's 0.5·Σ/B is mean((R - v)^2); slot 1 holds Σ adv·logp.
PPO_API int ppo_heads_train_a2c(const float* feat, const float* feat_v, int B, int H, const float* wc,
                                const float* bc, const float* wa, const float* ba, int A, const int64_t* idx,
                                long long row0, const int64_t* actions, const float* ret, float value_coef,
                                float entropy_coef, float inv_b, int feat_act, float* dfeat, float* dfeat_v,
                                float* part_w, float* part_b, float* part_loss, void* stream) {
  return cat_train("ppo_heads_train_a2c", LOSS_A2C, feat, feat_v, B, H, wc, bc, wa, ba, A, idx, row0, actions, nullptr,
                   nullptr, nullptr, ret, 0.f, value_coef, entropy_coef, inv_b, 0, feat_act, dfeat, dfeat_v, part_w,
                   part_b, part_loss, stream);
}

// Σ over the heads_train blocks (fixed order) -> head gradients; losses -> loss_acc
// (heads_reduce, which also says how slot 0 comes out as either algorithm's value loss)
PPO_API int ppo_heads_reduce(const float* part_w, const float* part_b, const float* part_loss, int nblk, int H, int A,
                             float* g_wc, float* g_bc, float* g_wa, float* g_ba, double* loss_acc, double inv_b,
                             float scale, int use_clipped_value_loss, void* stream) {
  (void)use_clipped_value_loss;  // both value losses are 0.5·mean(·)
  ProfScope prof("heads_reduce", as_stream(stream), 4.0 * nblk * (1.0 + A) * (H + 1));
  return heads_reduce(part_w, part_b, 1 + A, part_loss, nblk, H, A, g_wc, g_bc, g_wa, g_ba, loss_acc, inv_b, scale,
                      stream);
}

PPO_API int ppo_mean_f32(const float* x, long long n, float* out, void* stream) {
  PPO_REQUIRE(n > 0, "ppo_mean_f32: n=%lld", n);
  mean_kernel<<<1, 256, 0, as_stream(stream)>>>(x, n, out);
  PPO_LAUNCH_CHECK("mean_kernel");
  return 0;
}
