// Device pieces shared by the Categorical (heads.hip), DiagGaussian (heads_gauss.hip)
// and Bernoulli (heads_bern.hip) head kernels: the per-lane head-weight registers, the
// 1 + A wave-reduced dot products, the sampling counter's source, the activation
// gradient, the loss kinds with PPO's and A2C's row loss, the per-row storage scalars
// of the two float-action families and the loss-partial reduction.  The host side
// (kernel selection, reduce) is heads_dispatch.h.
#pragma once
#include "common.h"

namespace {

constexpr int HW = 4;  // waves per block

template <int HC, int AMAX>
struct HeadW {
  float wc[HC];
  float wa[AMAX][HC];
};

template <int HC, int AMAX>
__device__ __forceinline__ void load_head_w(HeadW<HC, AMAX>& w, const float* __restrict__ wc,
                                            const float* __restrict__ wa, int A, int H, int lane) {
#pragma unroll
  for (int c = 0; c < HC; ++c) w.wc[c] = lane + 64 * c < H ? wc[lane + 64 * c] : 0.f;
#pragma unroll
  for (int o = 0; o < AMAX; ++o)
#pragma unroll
    for (int c = 0; c < HC; ++c) w.wa[o][c] = (o < A && lane + 64 * c < H) ? wa[o * H + lane + 64 * c] : 0.f;
}

// value (from fv) and logits (from f) of one row; all lanes end up with the totals
template <int HC, int AMAX>
__device__ __forceinline__ void head_dots(const HeadW<HC, AMAX>& w, const float (&f)[HC], const float (&fv)[HC],
                                          float& value, float (&z)[AMAX], float bc, const float* __restrict__ ba,
                                          int A) {
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < HC; ++c) v += fv[c] * w.wc[c];
  value = wave_sum(v) + bc;
#pragma unroll
  for (int o = 0; o < AMAX; ++o) {
    if (o < A) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < HC; ++c) s += f[c] * w.wa[o][c];
      z[o] = wave_sum(s) + ba[o];
    } else {
      z[o] = -INFINITY;
    }
  }
}

// The sampling counter of an act launch: the by-value argument, or, for the _dc entry
// points, the word in device memory that `p` names.  `p` is a kernel argument, so the
// read is one uniform load per wave; the kernels never write the word (ppo_rng_advance
// does, in a launch of its own).
__device__ __forceinline__ uint64_t rng_counter_of(const unsigned long long* __restrict__ p,
                                                   unsigned long long by_value) {
  return p ? *p : by_value;
}

// d(pre-activation) from d(output) for the activation that produced y
__device__ __forceinline__ float act_grad(float d, float y, int act) {
  if (act == 1) return y > 0.f ? d : 0.f;     // ReLU (threshold_backward)
  if (act == 2) return d * (1.0f - y * y);    // tanh
  return d;
}

// The row loss a train launch computes: the `loss_kind` field of the three *TrainArgs
// structs, a run-time flag like use_clipped_value_loss (wave-uniform branch, no
// instantiation doubled).
constexpr int LOSS_PPO = 0;   // clipped surrogate + (clipped) value loss  algo/ppo.py:61-81
constexpr int LOSS_A2C = 1;   // policy gradient + squared error           algo/a2c_acktr.py:48-51
// The register-weight train kernels take the kind as a last template argument LK as well:
// LOSS_RT reads the field (the branch above), a fixed kind compiles the other loss out.
// A few instantiations sit on a VGPR occupancy step, and the branch's three or four extra
// registers pushed them over it; those (each file's split_loss) are built once per kind
// instead, which leaves their PPO code what it was without the branch.
constexpr int LOSS_RT = -1;

template <int LK>
__device__ __forceinline__ int loss_kind_of(int field) {
  return LK == LOSS_RT ? field : LK;
}

// A2C's row loss (algo/a2c_acktr.py:48-51, 71-72) from the row's value v, log-prob lp
// and stored return R:
//   adv = R - v (one fp32 subtraction; detached, so no gradient reaches v through it)
//   value loss  (R - v)^2 .mean()      -> g_v    = value_coef · inv_b · 2 (v - R)   (no 0.5 in A2C)
//   action loss -(adv · lp).mean()     -> g_logp = -inv_b · adv
// The loss partials go through the reduce PPO uses (loss_reduce_kernel: 0.5·Σ/B, -Σ/B), so
// slot 0 accumulates 2 (R - v)^2 (the doubling is exact in fp32) and slot 1 adv · lp.
// Neither old_logp, the stored advantage nor the stored value prediction is used.
__device__ __forceinline__ void a2c_row_loss(float v, float lp, float R, float value_coef, float inv_b,
                                             float& g_logp, float& g_v, float& s_vl, float& s_al) {
  const float adv = R - v;
  g_logp = -inv_b * adv;
  g_v = value_coef * inv_b * (2.f * (v - R));
  s_vl += 2.f * (adv * adv);
  s_al += adv * lp;
}

// x of lane j, in every lane (j wave-uniform)
__device__ __forceinline__ float bcast(float x, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j));
}

// bcast(x, j) that is done where the value is converted to float, not where it is written
struct LaneOf {
  float x;
  int j;
  __device__ __forceinline__ operator float() const { return bcast(x, j); }
};

// PPO's row loss (algo/ppo.py:61-77) from the row's value v, log-prob lp and its stored
// advantage, old log-prob, value prediction vo and return R: clipped surrogate and the
// clipped or plain value loss, with autograd's tie conventions (0.5 each way) in g_logp, g_v.
// Args: a *TrainArgs.  F: float, or LaneOf in the Categorical kernels, which keep their
// three readlanes at the places of use below (hoisted to the call, the compiler schedules
// every one of their train kernels that has this branch differently).
template <class Args, class F>
__device__ __forceinline__ void ppo_row_loss(const Args& a, float v, float lp, F adv_of, F olp_of, F vo_of,
                                             float R, float& g_logp, float& g_v, float& s_vl, float& s_al) {
  const float clip = a.clip;
  // action loss (ppo.py:61-66)
  const float adv = adv_of;
  const float ratio = expf(lp - (float)olp_of);
  const float surr1 = ratio * adv;
  const float rc = fminf(fmaxf(ratio, 1.0f - clip), 1.0f + clip);
  const float surr2 = rc * adv;
  const float w1 = surr1 < surr2 ? 1.f : (surr1 == surr2 ? 0.5f : 0.f);
  const float inr = (ratio >= 1.0f - clip && ratio <= 1.0f + clip) ? 1.f : 0.f;
  g_logp = -a.inv_b * (w1 * adv + (1.f - w1) * adv * inr) * ratio;
  // value loss (ppo.py:68-77)
  const float vo = vo_of;
  float vl_row;
  if (a.use_clipped_value_loss) {
    const float dv = v - vo;
    const float vpc = vo + fminf(fmaxf(dv, -clip), clip);
    const float l1 = (v - R) * (v - R);
    const float l2 = (vpc - R) * (vpc - R);
    vl_row = fmaxf(l1, l2);
    const float u1 = l1 > l2 ? 1.f : (l1 == l2 ? 0.5f : 0.f);
    const float vin = (dv >= -clip && dv <= clip) ? 1.f : 0.f;
    g_v = a.value_coef * 0.5f * a.inv_b * (u1 * 2.f * (v - R) + (1.f - u1) * 2.f * (vpc - R) * vin);
  } else {
    vl_row = (R - v) * (R - v);
    g_v = a.value_coef * a.inv_b * (v - R);
  }
  s_vl += vl_row;
  s_al += fminf(surr1, surr2);
}

// Per-row storage scalars of the DiagGaussian and Bernoulli train kernels (Args: their
// *TrainArgs): the minibatch gather idx -> advantage, old log-prob, value, return of all
// of the wave's rows are fetched up front, lane j holding row r0 + j (rows_per_wave <= 64),
// and broadcast per row, so no row waits on two dependent loads.
struct RowScalars {
  float adv = 0.f, olp = 0.f, vo = 0.f, ret = 0.f;
  int sr_lo = 0, sr_hi = 0;   // storage row (the action plane is read per row, one row ahead)
  template <class Args>
  __device__ __forceinline__ void load(const Args& a, int loss_kind, long long r0, int lane) {
    if (lane < a.rows_per_wave && r0 + lane < a.B) {
      const long long sr = a.idx ? (long long)a.idx[r0 + lane] : a.row0 + r0 + lane;
      sr_lo = (int)(sr & 0xffffffffll);
      sr_hi = (int)(sr >> 32);
      if (loss_kind != LOSS_A2C) {   // A2C: the three pointers may be NULL
        adv = a.adv[sr];
        olp = a.old_logp[sr];
        vo = a.vpred[sr];
      }
      ret = a.ret[sr];
    }
  }
  __device__ __forceinline__ long long storage_row(int j) const {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane(sr_lo, j);
    const long long hi = __builtin_amdgcn_readlane(sr_hi, j);
    return (hi << 32) | (long long)lo;
  }
};

// loss partials -> acc[0..3] += {0.5·Σvl/B, -Σal/B, Σent/B, # bad actions} (double, fixed order)
// (slot 0 of a LOSS_A2C launch holds Σ 2 (R - v)^2, so 0.5·Σ/B is mean((R - v)^2) there)
__global__ __launch_bounds__(256) void loss_reduce_kernel(const float* __restrict__ part_loss, int nblk,
                                                          double* __restrict__ loss_acc, double inv_b) {
  __shared__ double r[4][256];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblk; b += 256)
    for (int q = 0; q < 4; ++q) acc[q] += (double)part_loss[(size_t)b * 4 + q];
  for (int q = 0; q < 4; ++q) r[q][threadIdx.x] = acc[q];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o)
      for (int q = 0; q < 4; ++q) r[q][threadIdx.x] += r[q][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss_acc[0] += 0.5 * r[0][0] * inv_b;
    loss_acc[1] += -r[1][0] * inv_b;
    loss_acc[2] += r[2][0] * inv_b;
    loss_acc[3] += r[3][0];
  }
}

// 64-column chunks per lane, rounded up to an instantiated count (1, 2, 4, 8)
static inline int hc_of(int H) {
  const int c = (H + 63) / 64;
  return c <= 1 ? 1 : c <= 2 ? 2 : c <= 4 ? 4 : 8;
}

}  // namespace
