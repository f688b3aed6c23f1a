// Actor-critic heads for MultiBinary action spaces: Bernoulli distribution and the
// PPO loss (the third sibling of heads.hip and heads_gauss.hip).
//
// Reference:
//   Bernoulli (linear -> FixedBernoulli(logits))  distributions.py:93-104
//   FixedBernoulli log_probs / entropy / mode  distributions.py:45-56
//     (torch Bernoulli(logits=z): probs = sigmoid(z), sample = bernoulli(probs)
//      = (u < probs) for u ~ U[0, 1), log_prob = -BCEWithLogits(z, a) summed over
//      the A dims, entropy = BCEWithLogits(z, probs) summed, mode = probs > 0.5)
//   Policy.act / evaluate_actions  model.py:54-79
//   PPO clipped surrogate + clipped value loss + entropy  algo/ppo.py:61-81
//
// Same layout as heads.hip: one wave per row, HW waves per block, lane l holds
// hidden columns l + 64c, the 1 + A head dot products are wave-reduced so every
// lane holds value and the A logits z_o.  With e = exp(-|z|):
//   softplus(-|z|) = log1p(e),  p = sigmoid(z) = z >= 0 ? 1/(1+e) : e/(1+e)
//   log_prob = Σ_o a_o z_o - max(z_o, 0) - log1p(e_o)
//   entropy  = Σ_o log1p(e_o) + |z_o| e_o/(1+e_o)
// both finite for any finite z.
//
// Training gradients (g_logp = dL/dlog_prob of the row, as in heads.hip):
//   dL/dz_o = g_logp (a_o - p_o) + (entropy_coef / B) z_o p_o (1 - p_o)
// The parameters are dist.linear, so the partial layouts are heads.hip's and
// ppo_heads_reduce sums them.
#include "heads_dispatch.h"

namespace {

// per-dimension terms of Bernoulli(logits = z)
struct BernT {
  float p;     // sigmoid(z); for z >= 0 this is torch's 1 / (1 + exp(-z)) operation for operation
  float small; // sigmoid(-|z|) = min(p, 1 - p)
  float sp;    // softplus(-|z|) = log1p(exp(-|z|))
  float ent;   // entropy of the dimension
};

__device__ __forceinline__ BernT bern_terms(float z) {
  const float az = fabsf(z);
  const float e = expf(-az);
  const float inv = 1.f / (1.f + e);
  const float small = e * inv;   // sigmoid(-|z|)
  BernT t;
  t.p = z >= 0.f ? inv : small;
  t.small = small;
  t.sp = log1pf(e);
  t.ent = t.sp + az * small;
  return t;
}

// one uniform in [0, 1) per (row, dimension) from the counter RNG: the top 24 bits
// of the hash heads_gauss.hip feeds to Box-Muller
__device__ __forceinline__ float uniform_noise(uint64_t seed, uint64_t counter, long long row, int o, int A) {
  const uint64_t h = mix64(seed ^ mix64(counter * 0x2545F4914F6CDD1Dull + (uint64_t)(row * A + o)));
  return (float)((uint32_t)(h >> 40)) * (1.0f / 16777216.0f);
}

struct ActArgs {
  const float *feat, *feat_v;
  int N, H, A;
  const float *wc, *bc, *wa, *ba;
  const float* noise;      // [N][A] uniform draws in [0, 1) (host replay) or NULL
  unsigned long long seed, counter;
  const unsigned long long* counter_p;   // the counter as a word in device memory, or NULL (by value)
  int deterministic;
  const float* given;      // [N][A] actions to evaluate or NULL
  float *value, *action, *logp, *entropy;
  int rows_per_wave;
};

// act / evaluate: value, action (sample | mode | given), log_prob, entropy
// FAST: A == AMAX, H == 64·HC, no separate critic features (compile-time bounds)
template <int HC, int AMAX, bool FAST>
__global__ __launch_bounds__(64 * HW) void bern_act_kernel(const ActArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = FAST ? 64 * HC : a.H, A = FAST ? AMAX : a.A;
  const float* const feat_v = FAST ? nullptr : a.feat_v;
  const uint64_t counter = rng_counter_of(a.counter_p, a.counter);
  HeadW<HC, AMAX> w;
  load_head_w(w, a.wc, a.wa, A, H, lane);
  const float b0 = a.bc[0];
  const long long r0 = ((long long)blockIdx.x * HW + wave) * a.rows_per_wave;
  for (int rr = 0; rr < a.rows_per_wave; ++rr) {
    const long long row = r0 + rr;
    if (row >= a.N) break;
    float f[HC], fv[HC];
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      const bool in = lane + 64 * c < H;
      f[c] = in ? a.feat[row * H + lane + 64 * c] : 0.f;
      fv[c] = feat_v ? (in ? feat_v[row * H + lane + 64 * c] : 0.f) : f[c];
    }
    float value, z[AMAX], act[AMAX];
    head_dots(w, f, fv, value, z, b0, a.ba, A);
    float lp = 0.f, ent = 0.f;
#pragma unroll
    for (int o = 0; o < AMAX; ++o) {
      act[o] = 0.f;
      if (o < A) {
        const BernT t = bern_terms(z[o]);
        if (a.given) {
          act[o] = a.given[row * A + o];
        } else if (a.deterministic) {
          act[o] = t.p > 0.5f ? 1.f : 0.f;   // torch.gt(probs, 0.5): p == 0.5 gives 0
        } else {
          const float u = a.noise ? a.noise[row * A + o] : uniform_noise(a.seed, counter, row, o, A);
          act[o] = u < t.p ? 1.f : 0.f;
        }
        lp += act[o] * z[o] - fmaxf(z[o], 0.f) - t.sp;
        ent += t.ent;
      }
    }
    if (lane == 0) {
      if (a.value) a.value[row] = value;
      if (a.logp) a.logp[row] = lp;
      if (a.entropy) a.entropy[row] = ent;
    }
    if (a.action && lane < A) {
      float v = 0.f;   // act[lane] as a sum of one term and zeros (see bern_row)
#pragma unroll
      for (int o = 0; o < AMAX; ++o) v += lane == o ? act[o] : 0.f;
      a.action[row * A + lane] = v;
    }
  }
}

struct BernTrainArgs {
  const float* feat;       // [B][H] policy features
  const float* feat_v;     // [B][H] critic features (MLPBase) or NULL (= feat)
  int B, H, A;
  const float *wc, *bc, *wa, *ba;
  const int64_t* idx;      // storage row of each sample (nullable: row0 + b)
  long long row0;
  const float* actions;    // storage plane [row][A]
  const float *old_logp, *adv, *vpred, *ret;   // LOSS_A2C reads only ret; the other three may be NULL
  float clip, value_coef, entropy_coef, inv_b;
  int use_clipped_value_loss;
  int loss_kind;           // LOSS_PPO | LOSS_A2C (heads_common.h)
  int feat_act;            // activation producing the features: 0 none (GRU), 1 ReLU, 2 tanh
  float* dfeat;            // [B][H]
  float* dfeat_v;          // [B][H] critic-branch gradient (MLPBase) or NULL
  float* part_w;           // [blocks][1+A][H]: critic, logits
  float* part_b;           // [blocks][1+A]: critic bias, logit biases
  float* part_loss;        // [blocks][4]: Σ max(l1,l2), Σ min(s1,s2), Σ H, # rows with a component not 0 or 1
  int rows_per_wave;
};

// Loss terms and head gradients of one row.  The per-dimension terms (one expf, one
// log1pf and one division each) are computed once, by lane o for dimension o: that
// lane already holds the row's a_o.  The sums over o and the A gradients are then
// read lane by lane in ascending o, so every lane ends up with the same values; the
// row loss of the launch's kind is heads_common.h's.
template <int AMAX>
__device__ __forceinline__ void bern_row(const BernTrainArgs& a, int loss_kind, int A, int lane, float value,
                                         const float (&z)[AMAX], float acur, float adv, float olp, float vo, float R,
                                         float& g_v, float (&gz)[AMAX], float& s_vl, float& s_al, float& s_ent,
                                         float& s_bad) {
  const float ec = a.entropy_coef * a.inv_b;
  // this lane's logit (lanes >= A: 0, their results are never read).  A sum of one
  // term and zeros, not a chain of selects: the compiler turns such a chain into a
  // lane-indexed load from a scratch copy of z
  float zl = 0.f;
#pragma unroll
  for (int o = 0; o < AMAX; ++o) zl += (o < A && lane == o) ? z[o] : 0.f;
  const float al = lane < A ? acur : 0.f;
  const bool bad = __builtin_amdgcn_ballot_w64(lane < A && !(al == 0.f || al == 1.f)) != 0;   // NaN included
  const BernT t = bern_terms(zl);
  const float lpl = al * zl - fmaxf(zl, 0.f) - t.sp;
  float lp = 0.f, ent = 0.f;
#pragma unroll
  for (int o = 0; o < AMAX; ++o) {
    if (o < A) {
      lp += bcast(lpl, o);
      ent += bcast(t.ent, o);
    }
  }
  s_bad += bad ? 1.f : 0.f;   // counted; PPO.update raises
  s_ent += ent;
  float g_logp;
  if (loss_kind == LOSS_A2C) {
    a2c_row_loss(value, lp, R, a.value_coef, a.inv_b, g_logp, g_v, s_vl, s_al);   // a2c_acktr.py:48-51
  } else {
    ppo_row_loss(a, value, lp, adv, olp, vo, R, g_logp, g_v, s_vl, s_al);   // ppo.py:61-77
  }
  // p and p (1 - p) from sigmoid(-|z|), without cancellation
  const float amp = zl >= 0.f ? (al - 1.f) + t.small : al - t.small;   // a_o - p_o
  const float gzl = g_logp * amp + ec * zl * (t.small * (1.f - t.small));
#pragma unroll
  for (int o = 0; o < AMAX; ++o) gz[o] = o < A ? bcast(gzl, o) : 0.f;
}

// head-bias / loss partials of the block: redb[wave] = {gbc, gba[AMAX], Σvl, Σal,
// Σent, #bad} summed over the HW waves in a fixed order (heads.hip's part_b layout)
template <int AMAX>
__device__ __forceinline__ void bern_store_scalars(const BernTrainArgs& a, int A, float (&redb)[HW][AMAX + 5],
                                                   int lane, int wave, float gbc, const float (&gba)[AMAX],
                                                   float s_vl, float s_al, float s_ent, float s_bad) {
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
  const int t = threadIdx.x, NO = 1 + A;
  if (t < NO) {
    float s = 0.f;
    for (int q = 0; q < HW; ++q) s += redb[q][t];
    a.part_b[(size_t)blockIdx.x * NO + t] = s;
  }
  if (t < 4) {
    float s = 0.f;
    for (int q = 0; q < HW; ++q) s += redb[q][AMAX + 1 + t];
    a.part_loss[(size_t)blockIdx.x * 4 + t] = s;
  }
}

// FAST: A == AMAX, H == 64·HC, no separate critic features / gradient
// LK: LOSS_RT, or the loss kind fixed at compile time (split_loss, heads_common.h)
template <int HC, int AMAX, bool FAST, int LK>
__global__ __launch_bounds__(64 * HW) void bern_train_kernel(const BernTrainArgs a) {
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
  RowScalars q;
  q.load(a, loss_kind, r0, lane);
  // features and the row's A action floats (lane o holds dimension o) one row ahead
  float fn[HC], fvn[HC], an = 0.f;
  auto load_row = [&](int rr) {
    const long long row = r0 + rr;
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      const bool in = row < a.B && lane + 64 * c < H;
      fn[c] = in ? a.feat[row * H + lane + 64 * c] : 0.f;
      fvn[c] = feat_v ? (in ? feat_v[row * H + lane + 64 * c] : 0.f) : fn[c];
    }
    if (row < a.B) {
      const long long sr = q.storage_row(rr);
      if (lane < A) an = a.actions[sr * A + lane];
    }
  };
  load_row(0);
  for (int rr = 0; rr < a.rows_per_wave; ++rr) {
    const long long row = r0 + rr;
    if (row >= a.B) break;
    float f[HC], fv[HC];
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      f[c] = fn[c];
      fv[c] = fvn[c];
    }
    const float acur = an;
    if (rr + 1 < a.rows_per_wave) load_row(rr + 1);
    float value, z[AMAX];
    head_dots(w, f, fv, value, z, b0, a.ba, A);
    float g_v, gz[AMAX];
    bern_row(a, loss_kind, A, lane, value, z, acur, bcast(q.adv, rr), bcast(q.olp, rr), bcast(q.vo, rr), bcast(q.ret, rr), g_v, gz,
             s_vl, s_al, s_ent, s_bad);
    // dL/dh for this lane's columns, through the features' activation; head grads
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      const float dv = g_v * w.wc[c];
      float d = dfeat_v ? 0.f : dv;
#pragma unroll
      for (int o = 0; o < AMAX; ++o) d += gz[o] * w.wa[o][c];
      if (lane + 64 * c < H) {
        const size_t p = (size_t)row * H + lane + 64 * c;
        a.dfeat[p] = act_grad(d, f[c], a.feat_act);
        if (dfeat_v) dfeat_v[p] = act_grad(dv, fv[c], a.feat_act);
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
      for (int p = 0; p < AMAX; ++p)
        if (o == p + 1) v = gwa[p][c];
      red[wave][lane + 64 * c] = v;
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int c = 0; c < HC; ++c) {
        const int j = lane + 64 * c;
        float s = red[0][j];
        for (int p = 1; p < HW; ++p) s += red[p][j];
        if (j < H) a.part_w[((size_t)blockIdx.x * NO + o) * H + j] = s;
      }
    }
    __syncthreads();
  }
  bern_store_scalars<AMAX>(a, A, redb, lane, wave, gbc, gba, s_vl, s_al, s_ent, s_bad);
}

// bern_train_kernel at H = 512, A = 8 (the FAST case) with the head weights in
// LDS, as heads_train_lds_kernel: a lane holds the columns 4·lane + q + 256·c2 and
// reads the 9 weight rows of those columns as ds_read_b128.  The register version
// keeps 72 weight VGPRs next to 72 gradient accumulators (one wave per SIMD).
__global__ __launch_bounds__(64 * HW) void bern_train_lds_kernel(const BernTrainArgs a) {
  constexpr int A = 8, H = 512;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ f32x4 Wl[9][128];   // row 0: critic, rows 1..8: logits
  for (int i = threadIdx.x; i < 9 * H; i += 64 * HW) {
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
  RowScalars q;
  q.load(a, a.loss_kind, r0, lane);
  f32x4 fn[2];
  float an = 0.f;
  auto load_row = [&](int rr) {
    const long long row = r0 + rr;
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2)
      fn[c2] = row < a.B ? reinterpret_cast<const f32x4*>(a.feat + row * H)[lane + 64 * c2] : f32x4{0.f, 0.f, 0.f, 0.f};
    if (row < a.B) {
      const long long sr = q.storage_row(rr);
      if (lane < A) an = a.actions[sr * A + lane];
    }
  };
  load_row(0);
  for (int rr = 0; rr < a.rows_per_wave; ++rr) {
    const long long row = r0 + rr;
    if (row >= a.B) break;
    const f32x4 f[2] = {fn[0], fn[1]};
    const float acur = an;
    if (rr + 1 < a.rows_per_wave) load_row(rr + 1);
    float dots[9];
#pragma unroll
    for (int o = 0; o < 9; ++o) {
      float t = 0.f;
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        const f32x4 w = Wl[o][lane + 64 * c2];
#pragma unroll
        for (int p = 0; p < 4; ++p) t += f[c2][p] * w[p];
      }
      dots[o] = wave_sum(t);
    }
    const float value = dots[0] + b0;
    float z[A];
#pragma unroll
    for (int o = 0; o < A; ++o) z[o] = dots[1 + o] + ba[o];
    float g[9], gz[A];   // g[0] = dL/dvalue, g[1 + o] = dL/dz_o
    bern_row(a, a.loss_kind, A, lane, value, z, acur, bcast(q.adv, rr), bcast(q.olp, rr), bcast(q.vo, rr), bcast(q.ret, rr), g[0], gz,
             s_vl, s_al, s_ent, s_bad);
#pragma unroll
    for (int o = 0; o < A; ++o) g[1 + o] = gz[o];
    // dL/dfeature of this lane's columns (through the activation), head gradients
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      f32x4 d = Wl[0][lane + 64 * c2] * g[0];
#pragma unroll
      for (int o = 1; o < 9; ++o) {
        const f32x4 w = Wl[o][lane + 64 * c2];
#pragma unroll
        for (int p = 0; p < 4; ++p) d[p] += g[o] * w[p];
      }
      f32x4 y;
#pragma unroll
      for (int p = 0; p < 4; ++p) y[p] = act_grad(d[p], f[c2][p], a.feat_act);
      reinterpret_cast<f32x4*>(a.dfeat + row * H)[lane + 64 * c2] = y;
#pragma unroll
      for (int o = 0; o < 9; ++o)
#pragma unroll
        for (int p = 0; p < 4; ++p) gw[o][c2][p] += g[o] * f[c2][p];
    }
    gbc += g[0];
#pragma unroll
    for (int o = 0; o < A; ++o) gba[o] += gz[o];
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
        for (int p = 1; p < HW; ++p) t += red[p][lane + 64 * c2];
        reinterpret_cast<f32x4*>(a.part_w + ((size_t)blockIdx.x * 9 + o) * H)[lane + 64 * c2] = t;
      }
    }
    __syncthreads();
  }
  bern_store_scalars<A>(a, A, redb, lane, wave, gbc, gba, s_vl, s_al, s_ent, s_bad);
}

// what heads_dispatch.h needs to know of this family
struct Bern {
  using Act = ActArgs;
  using Train = BernTrainArgs;
  static constexpr const char* noun = "action dimensions";
  static constexpr const char *act_scope = "heads_bern_act", *train_scope = "heads_bern_train";
  static constexpr const char *act_kernel = "bern_act_kernel", *train_kernel = "bern_train_kernel",
                              *train_lds_kernel = "bern_train_lds_kernel";
  static double act_row_bytes(const Act& a) { return 12.0 + 4.0 * a.A; }
  static double train_row_bytes(const Train& a) { return (a.loss_kind == LOSS_A2C ? 12.0 : 24.0) + 4.0 * a.A; }
  static constexpr bool split_loss(int HC, int AMAX, bool FAST) { return AMAX == 8 && HC == 4 && FAST; }
  template <int HC, int AMAX, bool FAST>
  static void launch_act(const Act& a, unsigned blocks, hipStream_t st) {
    bern_act_kernel<HC, AMAX, FAST><<<blocks, 64 * HW, 0, st>>>(a);
  }
  template <int HC, int AMAX, bool FAST, int LK>
  static void launch_train(const Train& a, int blocks, hipStream_t st) {
    bern_train_kernel<HC, AMAX, FAST, LK><<<blocks, 64 * HW, 0, st>>>(a);
  }
  static void launch_train_lds(const Train& a, int blocks, hipStream_t st) {
    bern_train_lds_kernel<<<blocks, 64 * HW, 0, st>>>(a);
  }
};

// ppo_heads_bern_act (counter_p NULL) / ppo_heads_bern_act_dc (the counter in device memory)
int bern_act(const char* name, const float* feat, const float* feat_v, int N, int H, const float* wc, const float* bc,
             const float* wa, const float* ba, int A, const float* noise, unsigned long long seed,
             unsigned long long counter, const unsigned long long* counter_p, int deterministic, const float* given,
             float* value, float* action, float* logp, float* entropy, void* stream) {
  const ActArgs a = {feat, feat_v, N, H, A, wc, bc, wa, ba, noise, seed, counter, counter_p,
                     deterministic, given, value, action, logp, entropy, /*rows_per_wave*/ 0};
  return heads_act<Bern>(name, a, stream);
}

// ppo_heads_bern_train (LOSS_PPO) / ppo_heads_bern_train_a2c (LOSS_A2C: old_logp, adv and vpred
// NULL, clip and use_clipped_value_loss 0, none of them read)
int bern_train(const char* name, int loss_kind, const float* feat, const float* feat_v, int B, int H, const float* wc,
               const float* bc, const float* wa, const float* ba, int A, const int64_t* idx, long long row0,
               const float* actions, const float* old_logp, const float* adv, const float* vpred, const float* ret,
               float clip, float value_coef, float entropy_coef, float inv_b, int use_clipped_value_loss,
               int feat_act, float* dfeat, float* dfeat_v, float* part_w, float* part_b, float* part_loss,
               void* stream) {
  const BernTrainArgs a = {feat, feat_v, B, H, A, wc, bc, wa, ba, idx, row0, actions, old_logp, adv, vpred,
                           ret, clip, value_coef, entropy_coef, inv_b, use_clipped_value_loss, loss_kind, feat_act,
                           dfeat, dfeat_v, part_w, part_b, part_loss, /*rows_per_wave*/ 0};
  return heads_train<Bern>(name, a, stream);
}

}  // namespace

// Policy.act / get_value / evaluate_actions heads for FixedBernoulli(logits):
//   given   != NULL: log_prob / entropy of the given [N][A] actions
//   deterministic: action = (sigmoid(z) > 0.5)
//   noise   != NULL: action = (noise < sigmoid(z)), noise uniform in [0, 1) (host-replay parity mode)
//   noise   == NULL: 24-bit uniforms from the counter RNG (seed, counter, row, o)
PPO_API int ppo_heads_bern_act(const float* feat, const float* feat_v, int N, int H, const float* wc, const float* bc,
                               const float* wa, const float* ba, int A, const float* noise, unsigned long long seed,
                               unsigned long long counter, int deterministic, const float* given, float* value,
                               float* action, float* logp, float* entropy, void* stream) {
  return bern_act("ppo_heads_bern_act", feat, feat_v, N, H, wc, bc, wa, ba, A, noise, seed, counter, nullptr,
                  deterministic, given, value, action, logp, entropy, stream);
}

// ppo_heads_bern_act with the counter in device memory (see ppo_heads_act_dc): one 8-byte
// word, read once per wave and never written
PPO_API int ppo_heads_bern_act_dc(const float* feat, const float* feat_v, int N, int H, const float* wc,
                                  const float* bc, const float* wa, const float* ba, int A, const float* noise,
                                  unsigned long long seed, const unsigned long long* counter, int deterministic,
                                  const float* given, float* value, float* action, float* logp, float* entropy,
                                  void* stream) {
  PPO_REQUIRE(counter != nullptr, "ppo_heads_bern_act_dc: counter is NULL (a device pointer to one 8-byte word)");
  return bern_act("ppo_heads_bern_act_dc", feat, feat_v, N, H, wc, bc, wa, ba, A, noise, seed, 0ull, counter,
                  deterministic, given, value, action, logp, entropy, stream);
}

// the Bernoulli ppo_heads_train: same launch shape (ppo_heads_train_blocks) and the
// same partial layouts, float actions [row][A]; ppo_heads_reduce sums the partials
PPO_API int ppo_heads_bern_train(const float* feat, const float* feat_v, int B, int H, const float* wc,
                                 const float* bc, const float* wa, const float* ba, int A, const int64_t* idx,
                                 long long row0, const float* actions, const float* old_logp, const float* adv,
                                 const float* vpred, const float* ret, float clip, float value_coef,
                                 float entropy_coef, float inv_b, int use_clipped_value_loss, int feat_act,
                                 float* dfeat, float* dfeat_v, float* part_w, float* part_b, float* part_loss,
                                 void* stream) {
  return bern_train("ppo_heads_bern_train", LOSS_PPO, feat, feat_v, B, H, wc, bc, wa, ba, A, idx, row0, actions,
                    old_logp, adv, vpred, ret, clip, value_coef, entropy_coef, inv_b, use_clipped_value_loss,
                    feat_act, dfeat, dfeat_v, part_w, part_b, part_loss, stream);
}

// ppo_heads_bern_train with A2C's row loss (algo/a2c_acktr.py:48-51, a2c_row_loss): reads
// only the actions and the returns of the storage; part_loss as ppo_heads_train_a2c
PPO_API int ppo_heads_bern_train_a2c(const float* feat, const float* feat_v, int B, int H, const float* wc,
                                     const float* bc, const float* wa, const float* ba, int A, const int64_t* idx,
                                     long long row0, const float* actions, const float* ret, float value_coef,
                                     float entropy_coef, float inv_b, int feat_act, float* dfeat, float* dfeat_v,
                                     float* part_w, float* part_b, float* part_loss, void* stream) {
  return bern_train("ppo_heads_bern_train_a2c", LOSS_A2C, feat, feat_v, B, H, wc, bc, wa, ba, A, idx, row0, actions,
                    nullptr, nullptr, nullptr, ret, 0.f, value_coef, entropy_coef, inv_b, 0, feat_act, dfeat,
                    dfeat_v, part_w, part_b, part_loss, stream);
}
