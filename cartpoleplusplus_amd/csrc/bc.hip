// The behaviour-cloning actor term (TD3+BC, Fujimoto & Gu 2021; cpp_ddpg_set_behaviour_cloning; an extension of ddpg_cartpole.py:111-113):
// on the GEMM levels this kernel stands behind the action-columns dX GEMM, which then runs with GE_NONE in place of GE_ACTOR_HEAD and
// leaves dQ/da alone.  With q_b = Q(s1_b, mu_b) of the head the actor follows (sel: the row's head under cpp_ddpg_set_actor_min_q):
//     m = (1 / B) sum_b |q_b|;   lambda = alpha / max(m, q_floor)
//     g_bi = -lambda dq_da_bi + (2 / A) (mu_bi - a_bi);   adz_bi = g_bi (1 - mu_bi^2)
// lambda needs every row, the head gradient is row-local: EVERY workgroup reduces all B values of |q| itself -- thread t takes rows t, t + 256,
// .. in order, f64, then one tree over the 256 partials in LDS -- so that all workgroups hold the same lambda to the bit with one launch, no
// atomics and no grid-wide wait (B values of L2-resident floats per workgroup).  Then a thread per row.
#include "common.h"

__global__ __launch_bounds__(BC_THREADS) void bc_kernel(const BcArgs s) {
  __shared__ double part[BC_THREADS];
  const int t = (int)threadIdx.x;
  double acc = 0.0;
  for (int i = t; i < s.B; i += BC_THREADS) {
    // (both heads' values are loaded and the VALUE is chosen: a choice between the two uniform pointers by the per-lane sel was compiled
    // into one scalar pointer for the whole wave -- every row read head 2)
    float q = s.q1[i];
    if (s.sel) { const float qb = s.q2[i]; q = s.sel[i] == 2 ? qb : q; }
    acc += (double)fabsf(q);
  }
  part[t] = acc;
  __syncthreads();
  for (int w = BC_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) part[t] += part[t + w];
    __syncthreads();
  }
  const float m = (float)(part[0] / (double)s.B);
  const float lambda = s.alpha / fmaxf(m, s.q_floor);      // (no gradient flows through lambda)
  if (blockIdx.x == 0 && t == 0) { s.stat[0] = lambda; s.stat[1] = m; }
  const int b = (int)blockIdx.x * BC_THREADS + t;
  if (b >= s.B) return;
  const int A = s.A;
  const float two_over_a = 2.f / (float)A;
  float sq = 0.f;
  for (int i = 0; i < A; ++i) {
    const long k = (long)b * A + i;
    const float mu = s.mu[k], diff = mu - s.act[k];
    const float g = two_over_a * diff - lambda * s.dq_da[k];
    s.g[k] = g;
    s.adz[k] = g * fmaf(-mu, mu, 1.f);
    sq = fmaf(diff, diff, sq);
  }
  s.rows[b] = sq / (float)A;
}

int launch_bc(cpp_ctx* ctx, const BcArgs& s) {
  if (s.B < 1 || s.A < 1 || !s.q1 || (s.sel && !s.q2) || !s.dq_da || !s.mu || !s.act || !s.adz || !s.stat || !s.g || !s.rows) {
    cpp_set_error("launch_bc: B %d, A %d", s.B, s.A);
    return 1;
  }
  prof_begin(ctx);
  hipLaunchKernelGGL(bc_kernel, dim3((s.B + BC_THREADS - 1) / BC_THREADS), dim3(BC_THREADS), 0, ctx->stream, s);
  LAUNCH_CHECK();
  prof_end(ctx, K_BC);
  return 0;
}
