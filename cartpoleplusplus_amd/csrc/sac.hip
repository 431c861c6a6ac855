// Soft actor-critic (Haarnoja et al. 2018): the row-local maths of a Gaussian tanh policy and its learned temperature -- an extension of
// the deterministic actor ddpg_cartpole.py:95-100, of its gradient :111-113 and of the critic's target :199-214.  The definition is
// include/cartpolepp_abi.h's (cpp_net_create_gaussian, cpp_ddpg_set_sac); tests/sac_np.py restates it.
//
// dist.hip's idiom: one wave per row, lane k holds action component k (A <= 64; lanes k >= A are idle), SAC_ROWS waves share a workgroup
// only for the temperature gradient's partial (SAC_ROWS doubles of LDS).  f32 operations are rounded one by one (the whole translation unit
// compiles with contraction off), expf / logf / log1pf / tanhf / cospif are the accurate ones, the sum over k is a wave-uniform loop that
// reads lane k's term with a readlane -- k ascending, the order a float32 restatement follows.  No atomics, no scratch.
#include "common.h"

#pragma clang fp contract(off)

constexpr int SAC_ROWS = 4;      // rows (waves) per workgroup: the partial count is dist.hip's, (B + 3) / 4 <= DDPG_HEADS_MAX_WGS

__device__ __forceinline__ float sac_bcast(float v, int j) {      // j is wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}
// ls = lo + 0.5 (hi - lo) (tanh(x) + 1); th: tanh(x), h: 0.5 (hi - lo)
__device__ __forceinline__ float sac_log_std(float th, float lo, float h) { return lo + h * (th + 1.f); }
// softplus(y) = max(y, 0) + log1p(exp(-|y|))
__device__ __forceinline__ float sac_softplus(float y) { return fmaxf(y, 0.f) + log1pf(expf(-fabsf(y))); }
// the unclipped Box-Muller z of tps_noise (common.h) on the words {row, stream + k, n_lo, n_hi}: stream 0x200 is the draw at state_1,
// 0x300 the draw at state_2 (A <= 64 keeps both apart from target policy smoothing's 0x100 + k)
__device__ __forceinline__ float sac_noise(unsigned stream, unsigned seed_lo, unsigned seed_hi, unsigned long long n, unsigned row, unsigned k) {
  const u32x4 r = philox4x32_10(u32x4{row, stream + k, (uint32_t)n, (uint32_t)(n >> 32)}, seed_lo, seed_hi);
  const float u1 = (float)((r.x >> 8) + 1u) * 0x1p-24f;      // (0, 1]: exact
  const float u2 = (float)(r.y >> 8) * 0x1p-24f;             // [0, 1): exact
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// jobs 1 and 2: a sample (n != nullptr) or the mean (eps = 0) of the policy whose head is `logits`, (B, 2A): m in columns [0, A), x in
// [A, 2A).  Writes eps, a (into a_out and, splice != nullptr, the critic's splice columns at their row stride) and logp; job 2
// (r_soft != nullptr) also r_soft = r - ((mask discount) alpha) logp with alpha = exp(*log_alpha)
__global__ __launch_bounds__(64 * SAC_ROWS) void sac_sample_kernel(SacSampleArgs s) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * SAC_ROWS + (threadIdx.x >> 6);
  if (b >= s.B) return;      // (wave-uniform)
  const int A = s.A;
  const bool on = lane < A;
  const unsigned long long n = s.n ? *s.n : 0ull;
  if (s.n_out && blockIdx.x == 0 && threadIdx.x == 0) *s.n_out = n;
  float term = 0.f;
  if (on) {
    const float m = s.logits[(long)b * 2 * A + lane], x = s.logits[(long)b * 2 * A + A + lane];
    const float h = 0.5f * (s.hi - s.lo);
    const float ls = sac_log_std(tanhf(x), s.lo, h);
    const float eps = s.n ? sac_noise(s.stream, s.seed_lo, s.seed_hi, n, (unsigned)b, (unsigned)lane) : 0.f;
    const float u = m + expf(ls) * eps;
    const float a = tanhf(u);
    const float corr = 2.f * ((0.69314718055994530942f - u) - sac_softplus(-2.f * u));
    term = (((-0.5f * (eps * eps)) - ls) - 0.91893853320467274178f) - corr;
    if (s.eps) s.eps[(long)b * A + lane] = eps;
    s.a_out[(long)b * A + lane] = a;
    if (s.splice) s.splice[(long)b * s.ld_splice + lane] = a;
    if (s.m_out) s.m_out[(long)b * A + lane] = m;
    if (s.ls_out) s.ls_out[(long)b * A + lane] = ls;
  }
  float logp = 0.f;
  for (int k = 0; k < A; ++k) logp = logp + sac_bcast(term, k);
  if (lane == 0) {
    if (s.logp) s.logp[b] = logp;
    if (s.r_soft) {
      const float alpha = expf(*s.log_alpha);
      s.r_soft[b] = s.r[b] - ((s.mask[b] * s.discount) * alpha) * logp;
    }
  }
}

// job 3: the actor's head gradient, (B, 2A), from dq = dQ/da, and the temperature gradient's per-workgroup partials
//   g_u = 2 alpha a - dq (1 - a^2);  d m = g_u;  d x = (g_u exp(ls) eps - alpha) * 0.5 (hi - lo) (1 - tanh(x)^2)
//   part[workgroup] = sum over its rows, in order, of (logp_b + Hbar), f64
__global__ __launch_bounds__(64 * SAC_ROWS) void sac_actor_grad_kernel(SacGradArgs s) {
  __shared__ double part[SAC_ROWS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.x * SAC_ROWS + wv;
  const int A = s.A;
  const float alpha = expf(*s.log_alpha);
  if (s.alpha_out && blockIdx.x == 0 && threadIdx.x == 0) *s.alpha_out = alpha;
  double t = 0.0;
  if (b < s.B) {      // (wave-uniform)
    if (lane < A) {
      const float x = s.logits[(long)b * 2 * A + A + lane];
      const float a = s.a[(long)b * A + lane], eps = s.eps[(long)b * A + lane], dq = s.dq_da[(long)b * A + lane];
      const float h = 0.5f * (s.hi - s.lo);
      const float th = tanhf(x);
      const float sd = expf(sac_log_std(th, s.lo, h));
      const float gu = ((2.f * alpha) * a) - dq * (1.f - a * a);
      s.dz[(long)b * 2 * A + lane] = gu;
      s.dz[(long)b * 2 * A + A + lane] = (((gu * sd) * eps) - alpha) * (h * (1.f - th * th));
    }
    t = (double)s.logp[b] + (double)s.target_entropy;
  }
  if (lane == 0) part[wv] = t;
  __syncthreads();
  if (s.part && threadIdx.x == 0) {      // (nullptr: an evaluation, which leaves the temperature's gradient alone)
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < SAC_ROWS; ++k) sum += part[k];
    s.part[blockIdx.x] = sum;
  }
}

// job 4: g_alpha = -(1 / B) sum of the partials in order, then Adam's element on log_alpha (TensorFlow's semantics through adam_rate:
// betas 0.9 / 0.999, epsilon 1e-8); w = {log_alpha, m, v, ..}.  One thread of one workgroup.
__global__ __launch_bounds__(64) void sac_temperature_kernel(const double* part, int nparts, int B, float lr, float* w, unsigned long long* step) {
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  for (int i = 0; i < nparts; ++i) sum += part[i];
  const float g = (float)(-(sum / (double)B));
  const unsigned long long t = *step + 1ull;
  const AdamElem e = adam_update(w[SAC_W_LOG_ALPHA], g, w[SAC_W_M], w[SAC_W_V], 1.f, adam_rate(lr, 0.9f, 0.999f, t), 0.9f, 0.999f, 1e-8f);
  w[SAC_W_LOG_ALPHA] = e.p; w[SAC_W_M] = e.m; w[SAC_W_V] = e.v;
  *step = t;
}

int sac_grid(int B) { return (B + SAC_ROWS - 1) / SAC_ROWS; }

int launch_sac_sample(cpp_ctx* ctx, const SacSampleArgs& s) {
  if (s.B < 1 || s.A < 1 || s.A > 64 || !s.logits || !s.a_out || (s.r_soft && !(s.log_alpha && s.r && s.mask && s.logp))) {
    cpp_set_error("launch_sac_sample: B %d, A %d", s.B, s.A);
    return 1;
  }
  prof_begin(ctx);
  hipLaunchKernelGGL(sac_sample_kernel, dim3(sac_grid(s.B)), dim3(64 * SAC_ROWS), 0, ctx->stream, s);
  LAUNCH_CHECK();
  prof_end(ctx, K_SAC);
  return 0;
}

int launch_sac_actor_grad(cpp_ctx* ctx, const SacGradArgs& s) {
  if (s.B < 1 || s.A < 1 || s.A > 64 || sac_grid(s.B) > DDPG_HEADS_MAX_WGS) { cpp_set_error("launch_sac_actor_grad: B %d, A %d", s.B, s.A); return 1; }
  prof_begin(ctx);
  hipLaunchKernelGGL(sac_actor_grad_kernel, dim3(sac_grid(s.B)), dim3(64 * SAC_ROWS), 0, ctx->stream, s);
  LAUNCH_CHECK();
  prof_end(ctx, K_SAC);
  return 0;
}

int launch_sac_temperature(cpp_ctx* ctx, const double* part, int B, float lr, float* w, uint64_t* step) {
  if (B < 1 || sac_grid(B) > DDPG_HEADS_MAX_WGS) { cpp_set_error("launch_sac_temperature: B %d", B); return 1; }
  prof_begin(ctx);
  hipLaunchKernelGGL(sac_temperature_kernel, dim3(1), dim3(64), 0, ctx->stream, part, sac_grid(B), B, lr, w, (unsigned long long*)step);
  LAUNCH_CHECK();
  prof_end(ctx, K_SAC);
  return 0;
}
