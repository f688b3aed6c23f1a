// The rollout's CNN trunk in one launch: conv1 -> conv2 -> conv3 forward as three
// phases of one persistent grid (one block per CU).  Every phase maps image b to
// block b mod G, so a block consumes only its own outputs of the phase before:
// no grid-wide synchronisation, only each wave's stores retired (vmcnt) and a
// block barrier between phases, then an agent-scope acquire (L1 invalidate).
// This removes the two kernel boundaries inside the trunk — 10.3-10.4 us each
// between these persistent kernels at the rollout's 4,096 images (c5 kernel trace,
// profiles/r05_l_c5_kernel_stats.csv) — and each phase is the unchanged kernel body
// (bit-identical outputs to the three launches).  The phases share one LDS buffer
// (the largest phase, conv2: 154,368 B).
#include "conv_launch.h"
#include "conv1_fwd_body.h"
#include "conv2_fwd_body.h"
#include "conv3_fwd_body.h"

namespace {

constexpr int max_of(int a, int b) { return a > b ? a : b; }
constexpr int TRUNK_LDS = max_of(max_of(C1F_LDS, C2F_LDS), max_of(C3C_LDS0, C3L_LDS));
static_assert(C2L_LDS <= TRUNK_LDS, "the trunk's conv2 lone tiles in the shared LDS");

__device__ __forceinline__ void trunk_phase_sync() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's output stores are in L2
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // no stale L1 line under the next phase's loads
}

// no ReLU mask bits: the masked (training) forward takes the three launches (ppo_trunk_fwd)
template <int NP>
__global__ __launch_bounds__(512) void trunk_fwd_kernel(const uint8_t* __restrict__ obs, const int64_t* __restrict__ idx,
                                                       long long row0, int B, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, float* __restrict__ a1,
                                                       const uint16_t* __restrict__ w2pl, const float* __restrict__ b2,
                                                       float* __restrict__ a2, const uint16_t* __restrict__ w3pl,
                                                       const float* __restrict__ b3, float* __restrict__ a3) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[TRUNK_LDS];
  conv1_fwd_bf16x3_body<4, false, NP == 1 ? 1 : 3>(obs, idx, row0, B, w1, b1, a1, nullptr,
                                                   reinterpret_cast<uint16_t (*)[4 * C1S]>(lds));
  trunk_phase_sync();
  conv2_fwd_x9c_body<NP, false, true>(a1, B, w2pl, b2, a2, nullptr, lds);
  trunk_phase_sync();
  conv3_fwd_c3_body<NP, 512>(a2, B, w3pl, b3, a3, lds);
}

}  // namespace

// conv1 -> conv2 -> conv3 forward (model.py:177-179) of u8 4-channel observation rows in
// one launch (trunk_fwd_kernel): a1, a2, a3 as ppo_conv1_fwd / ppo_conv2_fwd /
// ppo_conv3_fwd write them (bit-identical); m1 / m2 both NULL or both given (the
// ReLU mask bits of ppo_conv1_fwd_mask / ppo_conv2_fwd_mask).  Small batches (<=
// small_b), conv1_fwd tune 9 and the masked form take the three separate calls.
PPO_API int ppo_trunk_fwd(const uint8_t* obs, const int64_t* idx, long long row0, int B, const float* w1,
                          const float* b1, float* a1, uint32_t* m1, const float* w2p, const float* b2, float* a2,
                          uint64_t* m2, const float* w3p, const float* b3, float* a3, void* stream) {
  PPO_REQUIRE(B >= 0 && obs != nullptr && (m1 == nullptr) == (m2 == nullptr),
              "ppo_trunk_fwd: B=%d, obs and both-or-neither masks required", B);
  if (B == 0) return 0;
  // the masked (training) form runs the three launches: fused, its registers spill
  // (2 VGPRs at 256), and the training forward has 2 boundaries per minibatch only
  if (B <= tune_small_b() || tune_key(TK_CONV1_FWD) != 0 || m1 != nullptr) {
    int rc = m1 ? ppo_conv1_fwd_mask(obs, 1, idx, row0, 4, B, w1, b1, a1, m1, stream)
                : ppo_conv1_fwd(obs, 1, idx, row0, 4, B, w1, b1, a1, stream);
    if (rc == 0)
      rc = m2 ? ppo_conv2_fwd_mask(a1, B, w2p, b2, a2, m2, stream) : ppo_conv2_fwd(a1, B, w2p, b2, a2, stream);
    if (rc == 0) rc = ppo_conv3_fwd(a2, B, w3p, b3, a3, stream);
    return rc;
  }
  const unsigned nb = img_grid(B);
  hipStream_t st = as_stream(stream);
  int slot;
  const bool prof = ppo_prof_begin("trunk_fwd", st, &slot);
  const uint16_t* w2pl = planes_of(w2p, 64 * 512);
  const uint16_t* w3pl = planes_of(w3p, 32 * 576);
  PPO_LAUNCH_NP(trunk_fwd_kernel, nb, 512, st, obs, idx, row0, B, w1, b1, a1, w2pl, b2, a2, w3pl, b3, a3);
  if (prof) ppo_prof_end(slot, st, 2.0 * B * (400.0 * 32 * 256 + 81.0 * 64 * 512 + 49.0 * 32 * 576));
  PPO_LAUNCH_CHECK("trunk_fwd_kernel");
  return 0;
}
