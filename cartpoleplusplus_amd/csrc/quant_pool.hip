// Pooled twin quantile critics (Kuznetsov et al. 2020, TQC, with two heads on one representation): the atoms of both target heads are
// pooled, sorted, and the 2d largest of the pool are dropped; both online heads regress onto the kept ones -- an extension of the scalar
// critic ddpg_cartpole.py:166-177 and its target :199-214.  The definition is include/cartpolepp_abi.h's (cpp_net_create_pooled_quantile);
// tests/pool_np.py restates it.
//
// quant.hip's idiom, in a translation unit of its own: one wave per row, QPOOL_ROWS rows per workgroup, row sums are xor butterflies over
// the 64 lanes (offsets 32, 16, .. 1), f32 operations rounded one by one, f64 loss terms, the 21-stage bitonic network of __shfl_xor
// compare-exchanges for the sort, no LDS beyond the loss partials.  Lane l < N loads atom l of target head 1, lane N <= l < 2N atom l - N of
// target head 2, the others hold +inf (2N <= 64: N = 32 leaves no idle lane); after the sort lane j < M = 2N - 2d forms y_j once, lane
// i < N holds atom i of BOTH online heads, and one wave-uniform loop over j broadcasts y_j with a single readlane that feeds both heads'
// gradient and loss accumulators.
#include "common.h"

constexpr int QPOOL_ROWS = 4;      // rows (waves) per workgroup: the partial count is quant.hip's, (B + 3) / 4 <= DDPG_HEADS_MAX_WGS

__device__ __forceinline__ float qpool_mul(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float qpool_add(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}
__device__ __forceinline__ float qpool_sub(float x, float y) {
#pragma clang fp contract(off)
  return x - y;
}

__device__ __forceinline__ float qpool_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = qpool_add(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double qpool_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float qpool_bcast(float v, int j) {      // j is wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

// quant.hip's ascending bitonic sort of one value per lane across the wave (works on values: ties cannot change what any lane ends with)
__device__ __forceinline__ float qpool_sort(float v, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const float o = __shfl_xor(v, j, 64);
      const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
      v = keep_min ? fminf(v, o) : fmaxf(v, o);
    }
  }
  return v;
}

// the expect job: Q_k = (sum_i theta^k_i) / N of both heads on the actor-action evaluation, and the tops of the actor's objective
// Qbar = (Q_1 + Q_2) / 2 -- dz of BOTH q layers is 1 / (2N)
__global__ __launch_bounds__(64 * QPOOL_ROWS) void qpool_expect_kernel(const float* theta1, const float* theta2, int B, int N, float* q1_out,
                                                                        float* q2_out, float* dz1, float* dz2) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * QPOOL_ROWS + (threadIdx.x >> 6);
  if (b >= B) return;      // (wave-uniform)
  const bool on = lane < N;
  const long o = (long)b * N + lane;
  const float th1 = on ? theta1[o] : 0.f, th2 = on ? theta2[o] : 0.f;
  const float q1 = qpool_wave_sum(th1) / (float)N, q2 = qpool_wave_sum(th2) / (float)N;
  if (lane == 0) { q1_out[b] = q1; q2_out[b] = q2; }
  if (on) { const float top = 1.f / (float)(2 * N); dz1[o] = top; dz2[o] = top; }
}

struct QpoolTdArgs {
  const float *theta1, *theta2, *ttheta1, *ttheta2, *r, *mask, *w;      // w: importance weights (WEIGHTED instances only)
  float discount, kappa;
  int B, N, M;                                                          // M = 2N - 2d kept atoms of the pool, 2 <= M <= 2N
  float *q1_out, *q2_out, *tq1_out, *tq2_out, *theta1_out, *theta2_out, *sorted_out, *y_out, *td, *td2, *dz1, *dz2;      // dz1 == nullptr: an evaluation
  double* loss_part;      // [(B + QPOOL_ROWS - 1) / QPOOL_ROWS] per-workgroup sums of w_b (L^1_b + L^2_b), rows in order, head 1 before head 2
};

// the td job: both fed heads and the pooled target of one row -> Q_1, Q_2, Q_1', Q_2', the sorted pool, y_j = r* + g s_j (j < M),
// td_k = Q_k - mean_j y_j, both heads' gradients -(w_b / B) (1 / (N M)) sum_j |tau_i - [u^k_ij < 0]| clip(u^k_ij, -kappa, kappa) / kappa
// and the row's two quantile Huber losses into its workgroup's partial
template <bool WEIGHTED>
__device__ __forceinline__ void qpool_td_body(const QpoolTdArgs& a) {
  __shared__ double part[QPOOL_ROWS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.x * QPOOL_ROWS + wv;
  const int N = a.N, M = a.M;
  double wl = 0.0;
  if (b < a.B) {      // (wave-uniform)
    const bool on = lane < N, on2 = lane >= N && lane < 2 * N, kept = lane < M;
    const long o = (long)b * N + lane, op = (long)b * 2 * N + lane;
    const float th1 = on ? a.theta1[o] : 0.f, th2 = on ? a.theta2[o] : 0.f;
    const float z = on ? a.ttheta1[o] : (on2 ? a.ttheta2[o - N] : INFINITY);
    const float tq1 = qpool_wave_sum(on ? z : 0.f) / (float)N, tq2 = qpool_wave_sum(on2 ? z : 0.f) / (float)N;      // (before the sort)
    const float s = qpool_sort(z, lane);      // (the 2N atoms end in lanes 0 .. 2N-1: +inf sorts behind them)
    const float q1 = qpool_wave_sum(th1) / (float)N, q2 = qpool_wave_sum(th2) / (float)N;
    const float r = a.r[b], g = qpool_mul(a.mask[b], a.discount);
    const float y = kept ? qpool_add(r, qpool_mul(g, s)) : 0.f;      // lane j forms y_j once; the 2d largest atoms of the pool are dropped
    const float ym = qpool_wave_sum(y) / (float)M;
    const float tau = (float)(2 * lane + 1) / (float)(2 * N);
    const float kappa = a.kappa;
    const double kd = (double)kappa;
    float gs1 = 0.f, gs2 = 0.f;
    double ls1 = 0.0, ls2 = 0.0;
    for (int j = 0; j < M; ++j) {
      const float yj = qpool_bcast(y, j);
      const float u1 = qpool_sub(yj, th1), u2 = qpool_sub(yj, th2);
      const float k1 = fabsf(qpool_sub(tau, u1 < 0.f ? 1.f : 0.f)), k2 = fabsf(qpool_sub(tau, u2 < 0.f ? 1.f : 0.f));
      gs1 = qpool_add(gs1, qpool_mul(k1, fminf(fmaxf(u1, -kappa), kappa)));
      gs2 = qpool_add(gs2, qpool_mul(k2, fminf(fmaxf(u2, -kappa), kappa)));
      const double ud1 = (double)u1, au1 = fabs(ud1), ud2 = (double)u2, au2 = fabs(ud2);
      ls1 += (double)k1 * (au1 <= kd ? 0.5 * ud1 * ud1 : kd * (au1 - 0.5 * kd));
      ls2 += (double)k2 * (au2 <= kd ? 0.5 * ud2 * ud2 : kd * (au2 - 0.5 * kd));
    }
    const double nm = (double)N * (double)M;
    const double L1 = qpool_wave_sum(on ? ls1 : 0.0) / (kd * nm), L2 = qpool_wave_sum(on ? ls2 : 0.0) / (kd * nm);
    const float wb = WEIGHTED ? a.w[b] : 1.f;
    wl = WEIGHTED ? (double)wb * L1 + (double)wb * L2 : L1 + L2;      // (head 1's row loss before head 2's)
    if (lane == 0) {
      a.q1_out[b] = q1; a.q2_out[b] = q2; a.tq1_out[b] = tq1; a.tq2_out[b] = tq2;
      a.td[b] = qpool_sub(q1, ym); a.td2[b] = qpool_sub(q2, ym);
    }
    if (lane < 2 * N) { a.sorted_out[op] = s; a.y_out[op] = y; }
    if (on) {
      a.theta1_out[o] = th1; a.theta2_out[o] = th2;
      if (a.dz1) {
        const float inv_b = 1.f / (float)a.B, inv_nm = 1.f / (float)(N * M);
        const float d1 = -qpool_mul(gs1 / kappa, inv_nm), d2 = -qpool_mul(gs2 / kappa, inv_nm);
        a.dz1[o] = WEIGHTED ? qpool_mul(qpool_mul(d1, wb), inv_b) : qpool_mul(d1, inv_b);
        a.dz2[o] = WEIGHTED ? qpool_mul(qpool_mul(d2, wb), inv_b) : qpool_mul(d2, inv_b);
      }
    }
  }
  if (lane == 0) part[wv] = wl;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < QPOOL_ROWS; ++k) s += part[k];
    a.loss_part[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(64 * QPOOL_ROWS) void qpool_td_kernel(QpoolTdArgs a) { qpool_td_body<false>(a); }
__global__ __launch_bounds__(64 * QPOOL_ROWS) void qpool_td_weighted_kernel(QpoolTdArgs a) { qpool_td_body<true>(a); }

int launch_qpool_expect(cpp_ctx* ctx, const float* theta1, const float* theta2, int B, int N, float* q1_out, float* q2_out, float* dz1, float* dz2) {
  if (B < 1 || N < 2 || N > 32 || !theta1 || !theta2 || !q1_out || !q2_out || !dz1 || !dz2) { cpp_set_error("launch_qpool_expect: B %d, N %d", B, N); return 1; }
  prof_begin(ctx);
  hipLaunchKernelGGL(qpool_expect_kernel, dim3((B + QPOOL_ROWS - 1) / QPOOL_ROWS), dim3(64 * QPOOL_ROWS), 0, ctx->stream, theta1, theta2, B, N, q1_out,
                     q2_out, dz1, dz2);
  LAUNCH_CHECK();
  prof_end(ctx, K_QUANT);
  return 0;
}

int qpool_td_grid(int B) { return (B + QPOOL_ROWS - 1) / QPOOL_ROWS; }

int launch_qpool_td(cpp_ctx* ctx, const QpoolTdIo& io, const float* r, const float* mask, float discount, int B, int N, float kappa, int drop_per_head,
                    double* loss_part, const float* w) {
  if (B < 1 || N < 2 || N > 32 || drop_per_head < 0 || drop_per_head > N - 1 || !(kappa > 0.f) || qpool_td_grid(B) > DDPG_HEADS_MAX_WGS ||
      (io.dz1 == nullptr) != (io.dz2 == nullptr) || !io.theta1 || !io.theta2 || !io.ttheta1 || !io.ttheta2 || !r || !mask || !loss_part ||
      !io.q1_out || !io.q2_out || !io.tq1_out || !io.tq2_out || !io.theta1_out || !io.theta2_out || !io.sorted_out || !io.y_out || !io.td || !io.td2) {
    cpp_set_error("launch_qpool_td: B %d, N %d, drop %d per head, kappa %g", B, N, drop_per_head, (double)kappa);
    return 1;
  }
  QpoolTdArgs a;
  a.theta1 = io.theta1; a.theta2 = io.theta2; a.ttheta1 = io.ttheta1; a.ttheta2 = io.ttheta2; a.r = r; a.mask = mask; a.w = w;
  a.discount = discount; a.kappa = kappa;
  a.B = B; a.N = N; a.M = 2 * N - 2 * drop_per_head;
  a.q1_out = io.q1_out; a.q2_out = io.q2_out; a.tq1_out = io.tq1_out; a.tq2_out = io.tq2_out; a.theta1_out = io.theta1_out; a.theta2_out = io.theta2_out;
  a.sorted_out = io.sorted_out; a.y_out = io.y_out; a.td = io.td; a.td2 = io.td2; a.dz1 = io.dz1; a.dz2 = io.dz2;
  a.loss_part = loss_part;
  prof_begin(ctx);
  if (w) hipLaunchKernelGGL(qpool_td_weighted_kernel, dim3(qpool_td_grid(B)), dim3(64 * QPOOL_ROWS), 0, ctx->stream, a);
  else hipLaunchKernelGGL(qpool_td_kernel, dim3(qpool_td_grid(B)), dim3(64 * QPOOL_ROWS), 0, ctx->stream, a);
  LAUNCH_CHECK();
  prof_end(ctx, K_QUANT);
  return 0;
}
