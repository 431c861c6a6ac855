// The actor on the minimum head (cpp_ddpg_set_actor_min_q; an extension of ddpg_cartpole.py:111-113, :220-222) where the fused heads kernel
// does not run: on the GEMM levels both heads of a twin critic are evaluated at a = mu(s1), and this kernel stands between their q layers
// and the two dX chains.  Per row: sel = 1 if Q1 <= Q2 else 2 (a tie is head 1's); the chosen head's chain starts from 1, the other's from
// 0 -- the vectors that stand where the trainer's `ones` stands with the switch off -- so that a row's unselected head contributes exact
// zeros to dQ/da.
#include "common.h"

__global__ __launch_bounds__(256) void actor_min_kernel(const float* __restrict__ q1, const float* __restrict__ q2, int B, float* __restrict__ top1,
                                                        float* __restrict__ top2, int* __restrict__ sel) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= B) return;
  const bool first = q1[i] <= q2[i];
  top1[i] = first ? 1.f : 0.f;
  top2[i] = first ? 0.f : 1.f;
  sel[i] = first ? 1 : 2;
}

int launch_actor_min(cpp_ctx* ctx, const float* q1, const float* q2, int B, float* top1, float* top2, int* sel) {
  prof_begin(ctx);
  hipLaunchKernelGGL(actor_min_kernel, dim3((B + 255) / 256), dim3(256), 0, ctx->stream, q1, q2, B, top1, top2, sel);
  LAUNCH_CHECK();
  prof_end(ctx, K_ELEMENTWISE);
  return 0;
}
