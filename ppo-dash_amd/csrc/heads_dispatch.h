// Host side of the three heads families (heads.hip, heads_gauss.hip, heads_bern.hip):
// argument checks, launch shape and the choice of the kernel instantiation, written
// once over a per-family traits struct D, and the reduce of the train partials.
// The kernels stay per family; D names them.  D supplies
//   Act, Train                       the argument structs (fields N | B, H, A, feat_v,
//                                    rows_per_wave; Train also idx, loss_kind, feat, dfeat,
//                                    dfeat_v, part_w)
//   noun                             what A counts, for the act error text
//   act_scope, train_scope           ProfScope names
//   act_row_bytes, train_row_bytes   bytes per row next to the features (and idx)
//   act_kernel, train_kernel, train_lds_kernel   names for PPO_LAUNCH_CHECK
//   split_loss(HC, AMAX, FAST)       the instantiations built once per loss kind (LOSS_RT)
//   launch_act<HC, AMAX, FAST>, launch_train<HC, AMAX, FAST, LK>, launch_train_lds
#pragma once
#include "heads_common.h"
#include "tune.h"

namespace {

// FAST: A == AMAX, H == 64·HC, no separate critic features
template <class D, int HC, int AMAX>
int launch_act(const typename D::Act& a, hipStream_t st) {
  const unsigned blocks = ceil_div(a.N, HW * a.rows_per_wave);
  if (a.A == AMAX && a.H == 64 * HC && !a.feat_v)
    D::template launch_act<HC, AMAX, true>(a, blocks, st);
  else
    D::template launch_act<HC, AMAX, false>(a, blocks, st);
  PPO_LAUNCH_CHECK(D::act_kernel);
  return 0;
}

template <class D, int AMAX>
int dispatch_act(int HC, const typename D::Act& a, hipStream_t st) {
  switch (HC) {
    case 1: return launch_act<D, 1, AMAX>(a, st);
    case 2: return launch_act<D, 2, AMAX>(a, st);
    case 4: return launch_act<D, 4, AMAX>(a, st);
    case 8: return launch_act<D, 8, AMAX>(a, st);
  }
  ppo_set_error("heads: hidden size %d not supported (<= 512)", a.H);
  return PPO_EARG;
}

// a family's act / act_dc entry points after the latter's counter check
template <class D>
int heads_act(const char* name, typename D::Act a, void* stream) {
  PPO_REQUIRE(a.N >= 0 && a.A >= 1 && a.A <= 16, "%s: N=%d A=%d (1..16 %s)", name, a.N, a.A, D::noun);
  PPO_REQUIRE(a.H > 0 && a.H <= 512, "%s: hidden size %d (1..512)", name, a.H);
  ProfScope prof(D::act_scope, as_stream(stream),
                 (double)a.N * (4.0 * a.H * (a.feat_v ? 2 : 1) + D::act_row_bytes(a)));
  if (a.N == 0) return 0;
  // ~4096 waves in flight (4 per SIMD at the Categorical kernel's 122-137 VGPRs): a rollout batch
  // of 4,096 rows takes one row per wave, so no wave runs two rows' dependent chains back to back
  a.rows_per_wave = (int)std::min<long long>(8, std::max<long long>(1, ceil_div(a.N, 4096)));
  if (a.A <= 8) return dispatch_act<D, 8>(hc_of(a.H), a, as_stream(stream));
  return dispatch_act<D, 16>(hc_of(a.H), a, as_stream(stream));
}

template <class D, int HC, int AMAX, bool FAST>
void launch_train_reg(const typename D::Train& a, int blocks, hipStream_t st) {
  if constexpr (D::split_loss(HC, AMAX, FAST)) {
    if (a.loss_kind == LOSS_A2C)
      D::template launch_train<HC, AMAX, FAST, LOSS_A2C>(a, blocks, st);
    else
      D::template launch_train<HC, AMAX, FAST, LOSS_PPO>(a, blocks, st);
  } else {
    D::template launch_train<HC, AMAX, FAST, LOSS_RT>(a, blocks, st);
  }
}

// FAST: as launch_act, and no separate critic gradient.  The LDS-weight kernel takes
// FAST's H = 512, A = 8 case when its float4 accesses are aligned.
template <class D, int HC, int AMAX>
int launch_train(const typename D::Train& a, int blocks, hipStream_t st) {
  // ppo_tune_set("heads_lds", 0): the register-weight kernel (A/B)
  if (tune_heads_lds() && HC == 8 && AMAX == 8 && a.A == 8 && a.H == 512 && !a.feat_v && !a.dfeat_v &&
      ((uintptr_t)a.feat & 15) == 0 && ((uintptr_t)a.dfeat & 15) == 0 && ((uintptr_t)a.part_w & 15) == 0) {
    D::launch_train_lds(a, blocks, st);
    PPO_LAUNCH_CHECK(D::train_lds_kernel);
    return 0;
  }
  if (a.A == AMAX && a.H == 64 * HC && !a.feat_v && !a.dfeat_v)
    launch_train_reg<D, HC, AMAX, true>(a, blocks, st);
  else
    launch_train_reg<D, HC, AMAX, false>(a, blocks, st);
  PPO_LAUNCH_CHECK(D::train_kernel);
  return 0;
}

template <class D, int AMAX>
int dispatch_train(int HC, const typename D::Train& a, int blocks, hipStream_t st) {
  switch (HC) {
    case 1: return launch_train<D, 1, AMAX>(a, blocks, st);
    case 2: return launch_train<D, 2, AMAX>(a, blocks, st);
    case 4: return launch_train<D, 4, AMAX>(a, blocks, st);
    case 8: return launch_train<D, 8, AMAX>(a, blocks, st);
  }
  ppo_set_error("heads: hidden size %d not supported (<= 512)", a.H);
  return PPO_EARG;
}

// a family's train / train_a2c entry points: one argument check, launch shape and kernel
// selection; the two differ in the row loss and in the storage planes it reads
template <class D>
int heads_train(const char* name, typename D::Train a, void* stream) {
  PPO_REQUIRE(a.B > 0 && a.A >= 1 && a.A <= 16, "%s: B=%d A=%d", name, a.B, a.A);
  PPO_REQUIRE(a.H > 0 && a.H <= 512, "%s: hidden size %d (1..512)", name, a.H);
  ProfScope prof(D::train_scope, as_stream(stream),
                 (double)a.B * (8.0 * a.H * (a.feat_v ? 2 : 1) + (a.idx ? 8.0 : 0.0) + D::train_row_bytes(a)));
  a.rows_per_wave = 32;
  const int blocks = ppo_heads_train_blocks(a.B);
  if (a.A <= 8) return dispatch_train<D, 8>(hc_of(a.H), a, blocks, as_stream(stream));
  return dispatch_train<D, 16>(hc_of(a.H), a, blocks, as_stream(stream));
}

// Σ over the train blocks (fixed order) of part_w [blocks][1+A][H] and of the first 1 + A
// of part_b's NB columns -> head gradients; losses -> loss_acc.  part_loss slot 0 is halved
// (0.5·Σ/B): PPO's launches store Σ of the row's squared error there, the A2C ones
// Σ 2 (R - v)^2, so both come out as their algorithm's value loss.
int heads_reduce(const float* part_w, const float* part_b, long long NB, const float* part_loss, int nblk, int H,
                 int A, float* g_wc, float* g_bc, float* g_wa, float* g_ba, double* loss_acc, double inv_b,
                 float scale, void* stream) {
  const long long NO = 1 + A;
  int rc;
  if ((rc = ppo_colsum(part_w, NO * H, nblk, H, g_wc, scale, 0, stream))) return rc;
  if ((rc = ppo_colsum(part_w + H, NO * H, nblk, (long long)A * H, g_wa, scale, 0, stream))) return rc;
  if ((rc = ppo_colsum(part_b, NB, nblk, 1, g_bc, scale, 0, stream))) return rc;
  if ((rc = ppo_colsum(part_b + 1, NB, nblk, A, g_ba, scale, 0, stream))) return rc;
  if (loss_acc) {
    loss_reduce_kernel<<<1, 256, 0, as_stream(stream)>>>(part_loss, nblk, loss_acc, inv_b);
    PPO_LAUNCH_CHECK("loss_reduce_kernel");
  }
  return 0;
}

}  // namespace
