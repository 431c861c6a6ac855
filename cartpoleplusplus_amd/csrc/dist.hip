// Distributional (categorical) critic: Bellemare et al. 2017 ("C51") as the critic of D4PG (Barth-Maron et al. 2018) -- an extension of
// the scalar critic ddpg_cartpole.py:166-177 and its target :199-214.  The definition is include/cartpolepp_abi.h's
// (cpp_net_create_distributional); tests/dist_np.py restates it.
//
// One wave per row, lane i holds atom i (N <= 64; lanes i >= N are idle: -inf into a maximum, 0 into a sum).  Row maxima and sums are
// xor butterflies over the 64 lanes (offsets 32, 16, .. 1: every lane ends with the same bits, and a float32 restatement can follow the
// order).  The projection is a loop over j that broadcasts (p'_j, b_j) from lane j with a readlane at the uniform index j: no LDS, no
// atomics, one summation order.  DIST_ROWS waves share a workgroup only for the loss partial (DIST_ROWS doubles of LDS).
#include "common.h"

constexpr int DIST_ROWS = 4;      // rows (waves) per workgroup: the partial count is the heads kernel's, (B + 3) / 4 <= DDPG_HEADS_MAX_WGS

// f32 operations rounded one by one, never contracted into an FMA (as gather_body.h's n-step fold): the support, b, the triangular
// weight and the accumulation of m keep the order the definition states
__device__ __forceinline__ float dist_mul(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float dist_add(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}
__device__ __forceinline__ float dist_sub(float x, float y) {
#pragma clang fp contract(off)
  return x - y;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = dist_add(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float lane_bcast(float v, int j) {      // j is wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

// p = softmax(row) with the maximum subtracted first, Q = sum p z; lsm (optional) = log p.  Idle lanes: p = 0, lsm = 0.
__device__ __forceinline__ float dist_softmax(const float* row, int lane, int N, float z, float* q, float* lsm) {
  const bool on = lane < N;
  const float x = on ? row[lane] : -INFINITY;
  const float mx = wave_max(x);
  const float c = on ? dist_sub(x, mx) : 0.f;
  const float e = on ? expf(c) : 0.f;
  const float s = wave_sum(e);
  const float p = e / s;
  if (lsm) *lsm = on ? dist_sub(c, logf(s)) : 0.f;
  *q = wave_sum(dist_mul(p, z));
  return p;
}

// job (a): Q and the gradient of the expectation, d Q / d logit_i = p_i (z_i - Q), on the actor-action evaluation (and Q alone for the
// forward entry points: dz == nullptr)
__global__ __launch_bounds__(64 * DIST_ROWS) void dist_expect_kernel(const float* logits, int B, int N, float v_min, float delta, float* q_out, float* dz) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * DIST_ROWS + (threadIdx.x >> 6);
  if (b >= B) return;      // (wave-uniform)
  const float z = dist_add(v_min, dist_mul((float)lane, delta));
  float q;
  const float p = dist_softmax(logits + (long)b * N, lane, N, z, &q, nullptr);
  if (lane == 0) q_out[b] = q;
  if (dz && lane < N) dz[(long)b * N + lane] = dist_mul(p, dist_sub(z, q));
}

struct DistTdArgs {
  const float *logits, *tlogits, *r, *mask, *w;      // w: importance weights (WEIGHTED instances only)
  float discount, v_min, v_max, delta;
  int B, N;
  float *q_out, *tq_out, *p_out, *tp_out, *m_out, *td, *dz;      // dz == nullptr: an evaluation (check_loss)
  double* loss_part;      // [(B + DIST_ROWS - 1) / DIST_ROWS] per-workgroup sums of w_b L_b, rows in order
};

// job (b): the fed and the target evaluation of one row -> Q, Q', the projected target m, td = Q - sum m z, the logit gradient
// (w_b / B) (p - m), and the row's cross-entropy into its workgroup's partial
template <bool WEIGHTED>
__device__ __forceinline__ void dist_td_body(const DistTdArgs& a) {
  __shared__ double part[DIST_ROWS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.x * DIST_ROWS + wv;
  const int N = a.N;
  double wl = 0.0;
  if (b < a.B) {      // (wave-uniform)
    const float z = dist_add(a.v_min, dist_mul((float)lane, a.delta));
    float q, tq, lsm;
    const float p = dist_softmax(a.logits + (long)b * N, lane, N, z, &q, &lsm);
    const float tp = dist_softmax(a.tlogits + (long)b * N, lane, N, z, &tq, nullptr);
    const float r = a.r[b], g = dist_mul(a.mask[b], a.discount);
    // lane j forms its own b_j once (Tz_j, the clamp, one correctly rounded division); the loop broadcasts (p'_j, b_j)
    const float tz = fminf(fmaxf(dist_add(r, dist_mul(g, z)), a.v_min), a.v_max);
    const float bl = dist_sub(tz, a.v_min) / a.delta;
    float m = 0.f;
    for (int j = 0; j < N; ++j) {
      const float pj = lane_bcast(tp, j), bj = lane_bcast(bl, j);
      const float k = fmaxf(0.f, dist_sub(1.f, fabsf(dist_sub(bj, (float)lane))));
      m = dist_add(m, dist_mul(pj, k));
    }
    if (lane >= N) m = 0.f;      // (an idle lane holds no atom: a b_j that the division rounds past N - 1 leaves nothing here)
    const float y = wave_sum(dist_mul(m, z));
    const double ce = -wave_sum(lane < N ? (double)m * (double)lsm : 0.0);
    const float wb = WEIGHTED ? a.w[b] : 1.f;
    wl = WEIGHTED ? (double)wb * ce : ce;
    if (lane == 0) { a.q_out[b] = q; a.tq_out[b] = tq; a.td[b] = dist_sub(q, y); }
    if (lane < N) {
      const long o = (long)b * N + lane;
      a.p_out[o] = p; a.tp_out[o] = tp; a.m_out[o] = m;
      if (a.dz) {
        const float inv_b = 1.f / (float)a.B, d = dist_sub(p, m);
        a.dz[o] = WEIGHTED ? dist_mul(dist_mul(d, wb), inv_b) : dist_mul(d, inv_b);
      }
    }
  }
  if (lane == 0) part[wv] = wl;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < DIST_ROWS; ++k) s += part[k];
    a.loss_part[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(64 * DIST_ROWS) void dist_td_kernel(DistTdArgs a) { dist_td_body<false>(a); }
__global__ __launch_bounds__(64 * DIST_ROWS) void dist_td_weighted_kernel(DistTdArgs a) { dist_td_body<true>(a); }

int launch_dist_expect(cpp_ctx* ctx, const float* logits, int B, int N, float v_min, float v_max, float* q_out, float* dz) {
  if (B < 1 || N < 2 || N > 64) { cpp_set_error("launch_dist_expect: B %d, N %d", B, N); return 1; }
  const float delta = (v_max - v_min) / (float)(N - 1);
  prof_begin(ctx);
  hipLaunchKernelGGL(dist_expect_kernel, dim3((B + DIST_ROWS - 1) / DIST_ROWS), dim3(64 * DIST_ROWS), 0, ctx->stream, logits, B, N, v_min, delta, q_out, dz);
  LAUNCH_CHECK();
  prof_end(ctx, K_DIST);
  return 0;
}

int dist_td_grid(int B) { return (B + DIST_ROWS - 1) / DIST_ROWS; }

int launch_dist_td(cpp_ctx* ctx, const float* logits, const float* tlogits, const float* r, const float* mask, float discount, int B, int N,
                   float v_min, float v_max, float* q_out, float* tq_out, float* p_out, float* tp_out, float* m_out, float* td, float* dz,
                   double* loss_part, const float* w) {
  if (B < 1 || N < 2 || N > 64 || dist_td_grid(B) > DDPG_HEADS_MAX_WGS) { cpp_set_error("launch_dist_td: B %d, N %d", B, N); return 1; }
  DistTdArgs a;
  a.logits = logits; a.tlogits = tlogits; a.r = r; a.mask = mask; a.w = w;
  a.discount = discount; a.v_min = v_min; a.v_max = v_max; a.delta = (v_max - v_min) / (float)(N - 1);
  a.B = B; a.N = N;
  a.q_out = q_out; a.tq_out = tq_out; a.p_out = p_out; a.tp_out = tp_out; a.m_out = m_out; a.td = td; a.dz = dz; a.loss_part = loss_part;
  prof_begin(ctx);
  if (w) hipLaunchKernelGGL(dist_td_weighted_kernel, dim3(dist_td_grid(B)), dim3(64 * DIST_ROWS), 0, ctx->stream, a);
  else hipLaunchKernelGGL(dist_td_kernel, dim3(dist_td_grid(B)), dim3(64 * DIST_ROWS), 0, ctx->stream, a);
  LAUNCH_CHECK();
  prof_end(ctx, K_DIST);
  return 0;
}
