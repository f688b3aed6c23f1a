// Actor-critic heads for Box action spaces: DiagGaussian distribution and the
// PPO loss (the continuous-control counterpart of heads.hip).
//
// Reference:
//   DiagGaussian (fc_mean + AddBias logstd)  distributions.py:71-86
//   FixedNormal sample / log_probs / entropy / mode  distributions.py:30-42
//     (torch Normal(loc, scale): sample = normal(loc, scale) = eps*scale + loc,
//      log_prob = -(a-loc)^2 / (2 scale^2) - log(scale) - log(sqrt(2 pi)),
//      entropy = 0.5 + 0.5 log(2 pi) + log(scale); both summed over the A dims)
//   Policy.act / evaluate_actions  model.py:54-79
//   PPO clipped surrogate + clipped value loss + entropy  algo/ppo.py:61-81
//
// Same layout as heads.hip: one wave per row, HW waves per block, lane l holds
// hidden columns l + 64c, the 1 + A head dot products are wave-reduced so every
// lane holds value and the A means.  s_o = logstd[o], sigma_o = expf(s_o).
//
// Training gradients (g_logp = dL/dlog_prob of the row, as in heads.hip):
//   dL/dmu_o = g_logp (a_o - mu_o) / sigma_o^2          (takes the logits' place)
//   dL/ds_o  = Σ_rows g_logp ((a_o - mu_o)^2 / sigma_o^2 - 1) - entropy_coef
// The entropy does not depend on the row (d mean(entropy)/d s_o = 1), so its
// term is added once per launch, by block 0.
#include "heads_dispatch.h"

namespace {

constexpr float kLogSqrt2Pi = 0.91893853320467274178f;   // log(sqrt(2 pi))
constexpr float kEntConst = 1.41893853320467274178f;     // 0.5 + 0.5 log(2 pi)

// per-dimension constants of Normal(·, exp(logstd)), in torch's operation order
template <int AMAX>
struct GaussC {
  float sig[AMAX];    // scale = exp(logstd)
  float lsig[AMAX];   // log(scale)
  float var2[AMAX];   // 2 scale^2
  float ivar[AMAX];   // 1 / scale^2
  float ent;          // Σ_o 0.5 + 0.5 log(2 pi) + log(scale)
};

template <int AMAX>
__device__ __forceinline__ void load_gauss_c(GaussC<AMAX>& g, const float* __restrict__ logstd, int A) {
  g.ent = 0.f;
#pragma unroll
  for (int o = 0; o < AMAX; ++o) {
    const float sig = o < A ? expf(logstd[o]) : 1.f;
    const float var = sig * sig;
    g.sig[o] = sig;
    g.lsig[o] = logf(sig);
    g.var2[o] = 2.f * var;
    g.ivar[o] = 1.f / var;
    if (o < A) g.ent += kEntConst + g.lsig[o];
  }
}

template <int AMAX>
__device__ __forceinline__ float gauss_logp(const GaussC<AMAX>& g, const float (&mu)[AMAX], const float (&a)[AMAX],
                                            int A) {
  float lp = 0.f;
#pragma unroll
  for (int o = 0; o < AMAX; ++o) {
    if (o < A) {
      const float d = a[o] - mu[o];
      lp += (-(d * d) / g.var2[o] - g.lsig[o]) - kLogSqrt2Pi;
    }
  }
  return lp;
}

// one standard normal per (row, dimension) from the counter RNG: Box-Muller on two
// 24-bit uniforms of one hash; u1 in (0, 1] keeps it finite (|eps| <= 5.77)
__device__ __forceinline__ float normal_noise(uint64_t seed, uint64_t counter, long long row, int o, int A) {
  const uint64_t h = mix64(seed ^ mix64(counter * 0x2545F4914F6CDD1Dull + (uint64_t)(row * A + o)));
  const float u1 = u01_open0(h), u2 = u01_open0(h << 24);
  return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// eps * sigma + mean as torch.normal(mean, std) = normal_().mul_(std).add_(mean)
// computes it: a rounded multiply, then a rounded add.  The rest of this file is
// compiled with contraction on, and HIP's __fmul_rn / __fadd_rn are plain operators
// that the compiler may fuse, hence the pragma.
__device__ __forceinline__ float mul_then_add(float eps, float sigma, float mean) {
#pragma clang fp contract(off)
  const float p = eps * sigma;
  return p + mean;
}

struct ActArgs {
  const float *feat, *feat_v;
  int N, H, A;
  const float *wc, *bc, *wa, *ba, *logstd;
  const float* noise;      // [N][A] standard normal draws (host replay) or NULL
  unsigned long long seed, counter;
  const unsigned long long* counter_p;   // the counter as a word in device memory, or NULL (by value)
  int deterministic;
  const float* given;      // [N][A] actions to evaluate or NULL
  float *value, *action, *logp, *entropy;
  int rows_per_wave;
};

// act / evaluate: value, action (sample | mean | given), log_prob, entropy
// FAST: A == AMAX, H == 64·HC, no separate critic features (compile-time bounds)
template <int HC, int AMAX, bool FAST>
__global__ __launch_bounds__(64 * HW) void gauss_act_kernel(const ActArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int H = FAST ? 64 * HC : a.H, A = FAST ? AMAX : a.A;
  const float* const feat_v = FAST ? nullptr : a.feat_v;
  const uint64_t counter = rng_counter_of(a.counter_p, a.counter);
  HeadW<HC, AMAX> w;
  load_head_w(w, a.wc, a.wa, A, H, lane);
  GaussC<AMAX> gc;
  load_gauss_c(gc, a.logstd, A);
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
    float value, mu[AMAX], act[AMAX];
    head_dots(w, f, fv, value, mu, b0, a.ba, A);
#pragma unroll
    for (int o = 0; o < AMAX; ++o) {
      act[o] = 0.f;
      if (o < A) {
        if (a.given) {
          act[o] = a.given[row * A + o];
        } else if (a.deterministic) {
          act[o] = mu[o];
        } else {
          const float eps = a.noise ? a.noise[row * A + o] : normal_noise(a.seed, counter, row, o, A);
          act[o] = mul_then_add(eps, gc.sig[o], mu[o]);
        }
      }
    }
    const float lp = gauss_logp(gc, mu, act, A);
    if (lane == 0) {
      if (a.value) a.value[row] = value;
      if (a.logp) a.logp[row] = lp;
      if (a.entropy) a.entropy[row] = gc.ent;
    }
    if (a.action && lane < A) {
      float v = act[0];
#pragma unroll
      for (int o = 1; o < AMAX; ++o)
        if (lane == o) v = act[o];
      a.action[row * A + lane] = v;
    }
  }
}

struct GaussTrainArgs {
  const float* feat;       // [B][H] policy features
  const float* feat_v;     // [B][H] critic features (MLPBase) or NULL (= feat)
  int B, H, A;
  const float *wc, *bc, *wa, *ba, *logstd;
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
  float* part_w;           // [blocks][1+A][H]: critic, means
  float* part_b;           // [blocks][1+2A]: critic bias, mean biases, logstd
  float* part_loss;        // [blocks][4]: Σ max(l1,l2), Σ min(s1,s2), Σ H, # rows with a non-finite action
  int rows_per_wave;
};

// Loss terms and head gradients of one row (every lane computes the same values):
// the row loss of the launch's kind (heads_common.h), then dL/dmu and the row's
// dL/dlogstd term added to gs.
template <int AMAX>
__device__ __forceinline__ void gauss_row(const GaussTrainArgs& a, int loss_kind, int A, const GaussC<AMAX>& gc, float value,
                                          const float (&mu)[AMAX], const float (&act)[AMAX], float adv, float olp,
                                          float vo, float R, float& g_v, float (&gmu)[AMAX], float (&gs)[AMAX],
                                          float& s_vl, float& s_al, float& s_bad) {
  bool bad = false;
#pragma unroll
  for (int o = 0; o < AMAX; ++o)
    if (o < A) bad |= !__builtin_isfinite(act[o]);
  s_bad += bad ? 1.f : 0.f;   // counted; PPO.update raises
  const float lp = gauss_logp(gc, mu, act, A);
  float g_logp;
  if (loss_kind == LOSS_A2C) {
    a2c_row_loss(value, lp, R, a.value_coef, a.inv_b, g_logp, g_v, s_vl, s_al);   // a2c_acktr.py:48-51
  } else {
    ppo_row_loss(a, value, lp, adv, olp, vo, R, g_logp, g_v, s_vl, s_al);   // ppo.py:61-77
  }
#pragma unroll
  for (int o = 0; o < AMAX; ++o) {
    if (o < A) {
      const float d = act[o] - mu[o];
      const float t = d * gc.ivar[o];
      gmu[o] = g_logp * t;
      gs[o] += g_logp * (d * t - 1.f);
    } else {
      gmu[o] = 0.f;
    }
  }
}

// head-bias / logstd / loss partials of the block: redb[wave] = {gbc, gba[AMAX],
// gs[AMAX], Σvl, Σal, Σent, #bad} summed over the HW waves in a fixed order
template <int AMAX>
__device__ __forceinline__ void gauss_store_scalars(const GaussTrainArgs& a, int A, float (&redb)[HW][2 * AMAX + 5],
                                                    int lane, int wave, float gbc, const float (&gba)[AMAX],
                                                    const float (&gs)[AMAX], float s_vl, float s_al, float s_ent,
                                                    float s_bad) {
  if (lane == 0) {
    redb[wave][0] = gbc;
#pragma unroll
    for (int o = 0; o < AMAX; ++o) {
      redb[wave][1 + o] = gba[o];
      redb[wave][1 + AMAX + o] = gs[o];
    }
    redb[wave][2 * AMAX + 1] = s_vl;
    redb[wave][2 * AMAX + 2] = s_al;
    redb[wave][2 * AMAX + 3] = s_ent;
    redb[wave][2 * AMAX + 4] = s_bad;
  }
  __syncthreads();
  const int t = threadIdx.x, NB = 1 + 2 * A;
  if (t < NB) {
    const int slot = t <= A ? t : 1 + AMAX + (t - 1 - A);
    float s = 0.f;
    for (int q = 0; q < HW; ++q) s += redb[q][slot];
    // d(-entropy_coef · mean(entropy))/d logstd_o = -entropy_coef: once per launch
    if (t > A && blockIdx.x == 0) s -= a.entropy_coef;
    a.part_b[(size_t)blockIdx.x * NB + t] = s;
  }
  if (t < 4) {
    float s = 0.f;
    for (int q = 0; q < HW; ++q) s += redb[q][2 * AMAX + 1 + t];
    a.part_loss[(size_t)blockIdx.x * 4 + t] = s;
  }
}

// FAST: A == AMAX, H == 64·HC, no separate critic features / gradient
// LK: LOSS_RT, or the loss kind fixed at compile time (split_loss, heads_common.h)
template <int HC, int AMAX, bool FAST, int LK>
__global__ __launch_bounds__(64 * HW) void gauss_train_kernel(const GaussTrainArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int loss_kind = loss_kind_of<LK>(a.loss_kind);
  const int H = FAST ? 64 * HC : a.H, A = FAST ? AMAX : a.A;
  const float* const feat_v = FAST ? nullptr : a.feat_v;
  float* const dfeat_v = FAST ? nullptr : a.dfeat_v;
  HeadW<HC, AMAX> w;
  load_head_w(w, a.wc, a.wa, A, H, lane);
  GaussC<AMAX> gc;
  load_gauss_c(gc, a.logstd, A);
  const float b0 = a.bc[0];
  float gwc[HC], gwa[AMAX][HC], gbc = 0.f, gba[AMAX], gs[AMAX];
#pragma unroll
  for (int c = 0; c < HC; ++c) gwc[c] = 0.f;
#pragma unroll
  for (int o = 0; o < AMAX; ++o) {
    gba[o] = gs[o] = 0.f;
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
    float value, mu[AMAX], act[AMAX];
    head_dots(w, f, fv, value, mu, b0, a.ba, A);
#pragma unroll
    for (int o = 0; o < AMAX; ++o) act[o] = bcast(acur, o);
    float g_v, gmu[AMAX];
    gauss_row(a, loss_kind, A, gc, value, mu, act, bcast(q.adv, rr), bcast(q.olp, rr), bcast(q.vo, rr), bcast(q.ret, rr), g_v,
              gmu, gs, s_vl, s_al, s_bad);
    s_ent += gc.ent;
    // dL/dh for this lane's columns, through the features' activation; head grads
#pragma unroll
    for (int c = 0; c < HC; ++c) {
      const float dv = g_v * w.wc[c];
      float d = dfeat_v ? 0.f : dv;
#pragma unroll
      for (int o = 0; o < AMAX; ++o) d += gmu[o] * w.wa[o][c];
      if (lane + 64 * c < H) {
        const size_t p = (size_t)row * H + lane + 64 * c;
        a.dfeat[p] = act_grad(d, f[c], a.feat_act);
        if (dfeat_v) dfeat_v[p] = act_grad(dv, fv[c], a.feat_act);
      }
      gwc[c] += g_v * fv[c];
#pragma unroll
      for (int o = 0; o < AMAX; ++o) gwa[o][c] += gmu[o] * f[c];
    }
    gbc += g_v;
#pragma unroll
    for (int o = 0; o < AMAX; ++o) gba[o] += gmu[o];
  }
  // block reduction of the head-gradient partials across the HW waves
  __shared__ float red[HW][64 * HC];
  __shared__ float redb[HW][2 * AMAX + 5];
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
  gauss_store_scalars<AMAX>(a, A, redb, lane, wave, gbc, gba, gs, s_vl, s_al, s_ent, s_bad);
}

// gauss_train_kernel at H = 512, A = 8 (the FAST case) with the head weights in
// LDS, as heads_train_lds_kernel: a lane holds the columns 4·lane + q + 256·c2 and
// reads the 9 weight rows of those columns as ds_read_b128.  The register version
// keeps 72 weight VGPRs next to 72 gradient accumulators (one wave per SIMD).
__global__ __launch_bounds__(64 * HW) void gauss_train_lds_kernel(const GaussTrainArgs a) {
  constexpr int A = 8, H = 512;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ f32x4 Wl[9][128];   // row 0: critic, rows 1..8: means
  for (int i = threadIdx.x; i < 9 * H; i += 64 * HW) {
    const int o = i / H, k = i - H * o;
    reinterpret_cast<float*>(&Wl[o][0])[k] = o == 0 ? a.wc[k] : a.wa[(o - 1) * H + k];
  }
  const float b0 = a.bc[0];
  float ba[A];
#pragma unroll
  for (int o = 0; o < A; ++o) ba[o] = a.ba[o];
  GaussC<A> gc;
  load_gauss_c(gc, a.logstd, A);
  __syncthreads();
  f32x4 gw[9][2];   // Σ_rows g_o · f (o = 0: critic), this lane's columns
#pragma unroll
  for (int o = 0; o < 9; ++o) gw[o][0] = gw[o][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  float gbc = 0.f, gba[A], gs[A];
#pragma unroll
  for (int o = 0; o < A; ++o) gba[o] = gs[o] = 0.f;
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
    float mu[A], act[A];
#pragma unroll
    for (int o = 0; o < A; ++o) {
      mu[o] = dots[1 + o] + ba[o];
      act[o] = bcast(acur, o);
    }
    float g[9], gmu[A];   // g[0] = dL/dvalue, g[1 + o] = dL/dmu_o
    gauss_row(a, a.loss_kind, A, gc, value, mu, act, bcast(q.adv, rr), bcast(q.olp, rr), bcast(q.vo, rr), bcast(q.ret, rr), g[0],
              gmu, gs, s_vl, s_al, s_bad);
    s_ent += gc.ent;
#pragma unroll
    for (int o = 0; o < A; ++o) g[1 + o] = gmu[o];
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
    for (int o = 0; o < A; ++o) gba[o] += gmu[o];
  }
  // block reduction of the head-gradient partials across the HW waves (fixed order)
  __shared__ f32x4 red[HW][128];
  __shared__ float redb[HW][2 * A + 5];
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
  gauss_store_scalars<A>(a, A, redb, lane, wave, gbc, gba, gs, s_vl, s_al, s_ent, s_bad);
}

// what heads_dispatch.h needs to know of this family
struct Gauss {
  using Act = ActArgs;
  using Train = GaussTrainArgs;
  static constexpr const char* noun = "action dimensions";
  static constexpr const char *act_scope = "heads_gauss_act", *train_scope = "heads_gauss_train";
  static constexpr const char *act_kernel = "gauss_act_kernel", *train_kernel = "gauss_train_kernel",
                              *train_lds_kernel = "gauss_train_lds_kernel";
  static double act_row_bytes(const Act& a) { return 12.0 + 4.0 * a.A; }
  static double train_row_bytes(const Train& a) { return (a.loss_kind == LOSS_A2C ? 12.0 : 24.0) + 4.0 * a.A; }
  static constexpr bool split_loss(int HC, int AMAX, bool FAST) { return AMAX == 8 && HC == 1 && !FAST; }
  template <int HC, int AMAX, bool FAST>
  static void launch_act(const Act& a, unsigned blocks, hipStream_t st) {
    gauss_act_kernel<HC, AMAX, FAST><<<blocks, 64 * HW, 0, st>>>(a);
  }
  template <int HC, int AMAX, bool FAST, int LK>
  static void launch_train(const Train& a, int blocks, hipStream_t st) {
    gauss_train_kernel<HC, AMAX, FAST, LK><<<blocks, 64 * HW, 0, st>>>(a);
  }
  static void launch_train_lds(const Train& a, int blocks, hipStream_t st) {
    gauss_train_lds_kernel<<<blocks, 64 * HW, 0, st>>>(a);
  }
};

// ppo_heads_gauss_act (counter_p NULL) / ppo_heads_gauss_act_dc (the counter in device memory)
int gauss_act(const char* name, const float* feat, const float* feat_v, int N, int H, const float* wc,
              const float* bc, const float* wa, const float* ba, const float* logstd, int A, const float* noise,
              unsigned long long seed, unsigned long long counter, const unsigned long long* counter_p,
              int deterministic, const float* given, float* value, float* action, float* logp, float* entropy,
              void* stream) {
  const ActArgs a = {feat, feat_v, N, H, A, wc, bc, wa, ba, logstd, noise, seed, counter, counter_p,
                     deterministic, given, value, action, logp, entropy, /*rows_per_wave*/ 0};
  return heads_act<Gauss>(name, a, stream);
}

// ppo_heads_gauss_train (LOSS_PPO) / ppo_heads_gauss_train_a2c (LOSS_A2C: old_logp, adv and vpred
// NULL, clip and use_clipped_value_loss 0, none of them read)
int gauss_train(const char* name, int loss_kind, const float* feat, const float* feat_v, int B, int H,
                const float* wc, const float* bc, const float* wa, const float* ba, const float* logstd, int A,
                const int64_t* idx, long long row0, const float* actions, const float* old_logp, const float* adv,
                const float* vpred, const float* ret, float clip, float value_coef, float entropy_coef, float inv_b,
                int use_clipped_value_loss, int feat_act, float* dfeat, float* dfeat_v, float* part_w, float* part_b,
                float* part_loss, void* stream) {
  const GaussTrainArgs a = {feat, feat_v, B, H, A, wc, bc, wa, ba, logstd, idx, row0, actions, old_logp, adv, vpred,
                            ret, clip, value_coef, entropy_coef, inv_b, use_clipped_value_loss, loss_kind, feat_act,
                            dfeat, dfeat_v, part_w, part_b, part_loss, /*rows_per_wave*/ 0};
  return heads_train<Gauss>(name, a, stream);
}

}  // namespace

// Policy.act / get_value / evaluate_actions heads for FixedNormal(mean, exp(logstd)):
//   given   != NULL: log_prob / entropy of the given [N][A] actions
//   deterministic: action = mean
//   noise   != NULL: action = noise * sigma + mean (host-replay parity mode)
//   noise   == NULL: standard normal noise from the counter RNG (seed, counter, row, o)
PPO_API int ppo_heads_gauss_act(const float* feat, const float* feat_v, int N, int H, const float* wc,
                                const float* bc, const float* wa, const float* ba, const float* logstd, int A,
                                const float* noise, unsigned long long seed, unsigned long long counter,
                                int deterministic, const float* given, float* value, float* action, float* logp,
                                float* entropy, void* stream) {
  return gauss_act("ppo_heads_gauss_act", feat, feat_v, N, H, wc, bc, wa, ba, logstd, A, noise, seed, counter, nullptr,
                   deterministic, given, value, action, logp, entropy, stream);
}

// ppo_heads_gauss_act with the counter in device memory (see ppo_heads_act_dc): one 8-byte
// word, read once per wave and never written
PPO_API int ppo_heads_gauss_act_dc(const float* feat, const float* feat_v, int N, int H, const float* wc,
                                   const float* bc, const float* wa, const float* ba, const float* logstd, int A,
                                   const float* noise, unsigned long long seed, const unsigned long long* counter,
                                   int deterministic, const float* given, float* value, float* action, float* logp,
                                   float* entropy, void* stream) {
  PPO_REQUIRE(counter != nullptr, "ppo_heads_gauss_act_dc: counter is NULL (a device pointer to one 8-byte word)");
  return gauss_act("ppo_heads_gauss_act_dc", feat, feat_v, N, H, wc, bc, wa, ba, logstd, A, noise, seed, 0ull, counter,
                   deterministic, given, value, action, logp, entropy, stream);
}

// the Gaussian ppo_heads_train: same launch shape (ppo_heads_train_blocks), float
// actions [row][A], part_b sized [blocks][1 + 2A]
PPO_API int ppo_heads_gauss_train(const float* feat, const float* feat_v, int B, int H, const float* wc,
                                  const float* bc, const float* wa, const float* ba, const float* logstd, int A,
                                  const int64_t* idx, long long row0, const float* actions, const float* old_logp,
                                  const float* adv, const float* vpred, const float* ret, float clip,
                                  float value_coef, float entropy_coef, float inv_b, int use_clipped_value_loss,
                                  int feat_act, float* dfeat, float* dfeat_v, float* part_w, float* part_b,
                                  float* part_loss, void* stream) {
  return gauss_train("ppo_heads_gauss_train", LOSS_PPO, feat, feat_v, B, H, wc, bc, wa, ba, logstd, A, idx, row0,
                     actions, old_logp, adv, vpred, ret, clip, value_coef, entropy_coef, inv_b,
                     use_clipped_value_loss, feat_act, dfeat, dfeat_v, part_w, part_b, part_loss, stream);
}

// ppo_heads_gauss_train with A2C's row loss (algo/a2c_acktr.py:48-51, a2c_row_loss): reads
// only the actions and the returns of the storage; part_loss as ppo_heads_train_a2c
PPO_API int ppo_heads_gauss_train_a2c(const float* feat, const float* feat_v, int B, int H, const float* wc,
                                      const float* bc, const float* wa, const float* ba, const float* logstd, int A,
                                      const int64_t* idx, long long row0, const float* actions, const float* ret,
                                      float value_coef, float entropy_coef, float inv_b, int feat_act, float* dfeat,
                                      float* dfeat_v, float* part_w, float* part_b, float* part_loss, void* stream) {
  return gauss_train("ppo_heads_gauss_train_a2c", LOSS_A2C, feat, feat_v, B, H, wc, bc, wa, ba, logstd, A, idx, row0,
                     actions, nullptr, nullptr, nullptr, ret, 0.f, value_coef, entropy_coef, inv_b, 0, feat_act,
                     dfeat, dfeat_v, part_w, part_b, part_loss, stream);
}

// Σ over the gauss_train blocks (fixed order) -> head and logstd gradients; losses -> loss_acc
PPO_API int ppo_heads_gauss_reduce(const float* part_w, const float* part_b, const float* part_loss, int nblk, int H,
                                   int A, float* g_wc, float* g_bc, float* g_wa, float* g_ba, float* g_logstd,
                                   double* loss_acc, double inv_b, float scale, void* stream) {
  ProfScope prof("heads_gauss_reduce", as_stream(stream), 4.0 * nblk * ((1.0 + A) * H + 1.0 + 2.0 * A));
  const long long NB = 1 + 2 * A;
  if (int rc = heads_reduce(part_w, part_b, NB, part_loss, nblk, H, A, g_wc, g_bc, g_wa, g_ba, loss_acc, inv_b, scale,
                            stream))
    return rc;
  return ppo_colsum(part_b + 1 + A, NB, nblk, A, g_logstd, scale, 0, stream);
}
