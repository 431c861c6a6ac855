// Quantile critic: quantile regression (Dabney et al. 2018, QR-DQN) with truncated targets (Kuznetsov et al. 2020, TQC, one network) -- an
// extension of the scalar critic ddpg_cartpole.py:166-177 and its target :199-214.  The definition is include/cartpolepp_abi.h's
// (cpp_net_create_quantile); tests/quant_np.py restates it.
//
// dist.hip's idiom: one wave per row, lane i holds atom i (N <= 64; lanes i >= N are idle: +inf into the sort, nothing into a sum), row
// sums are xor butterflies over the 64 lanes (offsets 32, 16, .. 1: every lane ends with the same bits, and a float32 restatement can
// follow the order), f32 operations rounded one by one.  The target atoms are sorted ascending across the lanes by a bitonic network of
// __shfl_xor compare-exchanges (21 stages, each lane keeps the minimum or the maximum by its lane bits: no LDS, no divergent branch); the
// N x M pairwise loss is a wave-uniform loop over j that broadcasts y_j from lane j with a readlane.  QUANT_ROWS waves share a workgroup
// only for the loss partial (QUANT_ROWS doubles of LDS).
#include "common.h"

constexpr int QUANT_ROWS = 4;      // rows (waves) per workgroup: the partial count is dist.hip's, (B + 3) / 4 <= DDPG_HEADS_MAX_WGS

__device__ __forceinline__ float quant_mul(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float quant_add(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}
__device__ __forceinline__ float quant_sub(float x, float y) {
#pragma clang fp contract(off)
  return x - y;
}

__device__ __forceinline__ float quant_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = quant_add(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double quant_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float quant_bcast(float v, int j) {      // j is wave-uniform
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

// ascending bitonic sort of one value per lane across the wave: blocks of k lanes alternate direction (the last stage, k = 64, is one
// ascending block), partners are j lanes apart; the lower lane of a pair keeps the minimum in an ascending block, the maximum in a
// descending one.  Works on values: ties cannot change what any lane ends with.
__device__ __forceinline__ float quant_sort(float v, int lane) {
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

// job (a): Q = (sum_i theta_i) / N and the gradient of the expectation, d Q / d theta_i = 1 / N, on the actor-action evaluation (and Q
// alone for the forward entry points: dz == nullptr)
__global__ __launch_bounds__(64 * QUANT_ROWS) void quant_expect_kernel(const float* theta, int B, int N, float* q_out, float* dz) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * QUANT_ROWS + (threadIdx.x >> 6);
  if (b >= B) return;      // (wave-uniform)
  const bool on = lane < N;
  const float th = on ? theta[(long)b * N + lane] : 0.f;
  const float q = quant_wave_sum(th) / (float)N;
  if (lane == 0) q_out[b] = q;
  if (dz && on) dz[(long)b * N + lane] = 1.f / (float)N;
}

struct QuantTdArgs {
  const float *theta, *ttheta, *r, *mask, *w;      // w: importance weights (WEIGHTED instances only)
  float discount, kappa;
  int B, N, M;                                     // M = N - (the dropped top target atoms), 1 <= M <= N
  float *q_out, *tq_out, *theta_out, *sorted_out, *y_out, *td, *dz;      // dz == nullptr: an evaluation (check_loss)
  double* loss_part;      // [(B + QUANT_ROWS - 1) / QUANT_ROWS] per-workgroup sums of w_b L_b, rows in order
};

// job (b): the fed and the target evaluation of one row -> Q, Q', the sorted target atoms, y_j = r + g s_j (j < M), td = Q - mean_j y_j,
// the gradient -(w_b / B) (1 / (N M)) sum_j |tau_i - [u_ij < 0]| clip(u_ij, -kappa, kappa) / kappa, and the row's quantile Huber loss
// into its workgroup's partial
template <bool WEIGHTED>
__device__ __forceinline__ void quant_td_body(const QuantTdArgs& a) {
  __shared__ double part[QUANT_ROWS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.x * QUANT_ROWS + wv;
  const int N = a.N, M = a.M;
  double wl = 0.0;
  if (b < a.B) {      // (wave-uniform)
    const bool on = lane < N, kept = lane < M;
    const long o = (long)b * N + lane;
    const float th = on ? a.theta[o] : 0.f;
    const float s = quant_sort(on ? a.ttheta[o] : INFINITY, lane);      // (the N atoms end in lanes 0 .. N-1: +inf sorts behind them)
    const float q = quant_wave_sum(th) / (float)N;
    const float tq = quant_wave_sum(on ? s : 0.f) / (float)N;
    const float r = a.r[b], g = quant_mul(a.mask[b], a.discount);
    const float y = kept ? quant_add(r, quant_mul(g, s)) : 0.f;          // lane j forms y_j once; the d largest atoms are dropped
    const float ym = quant_wave_sum(y) / (float)M;
    const float tau = (float)(2 * lane + 1) / (float)(2 * N);
    const float kappa = a.kappa;
    float gs = 0.f;
    double ls = 0.0;
    for (int j = 0; j < M; ++j) {
      const float yj = quant_bcast(y, j);
      const float u = quant_sub(yj, th);
      const float k = fabsf(quant_sub(tau, u < 0.f ? 1.f : 0.f));
      const float c = fminf(fmaxf(u, -kappa), kappa);
      gs = quant_add(gs, quant_mul(k, c));
      const double ud = (double)u, au = fabs(ud), kd = (double)kappa;
      const double h = au <= kd ? 0.5 * ud * ud : kd * (au - 0.5 * kd);
      ls += (double)k * h;
    }
    const double nm = (double)N * (double)M;
    const double L = quant_wave_sum(on ? ls : 0.0) / ((double)kappa * nm);
    const float wb = WEIGHTED ? a.w[b] : 1.f;
    wl = WEIGHTED ? (double)wb * L : L;
    if (lane == 0) { a.q_out[b] = q; a.tq_out[b] = tq; a.td[b] = quant_sub(q, ym); }
    if (on) {
      a.theta_out[o] = th; a.sorted_out[o] = s; a.y_out[o] = y;
      if (a.dz) {
        const float inv_b = 1.f / (float)a.B, inv_nm = 1.f / (float)(N * M);
        const float d = -quant_mul(gs / kappa, inv_nm);
        a.dz[o] = WEIGHTED ? quant_mul(quant_mul(d, wb), inv_b) : quant_mul(d, inv_b);
      }
    }
  }
  if (lane == 0) part[wv] = wl;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < QUANT_ROWS; ++k) s += part[k];
    a.loss_part[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(64 * QUANT_ROWS) void quant_td_kernel(QuantTdArgs a) { quant_td_body<false>(a); }
__global__ __launch_bounds__(64 * QUANT_ROWS) void quant_td_weighted_kernel(QuantTdArgs a) { quant_td_body<true>(a); }

int launch_quant_expect(cpp_ctx* ctx, const float* theta, int B, int N, float* q_out, float* dz) {
  if (B < 1 || N < 2 || N > 64) { cpp_set_error("launch_quant_expect: B %d, N %d", B, N); return 1; }
  prof_begin(ctx);
  hipLaunchKernelGGL(quant_expect_kernel, dim3((B + QUANT_ROWS - 1) / QUANT_ROWS), dim3(64 * QUANT_ROWS), 0, ctx->stream, theta, B, N, q_out, dz);
  LAUNCH_CHECK();
  prof_end(ctx, K_QUANT);
  return 0;
}

int quant_td_grid(int B) { return (B + QUANT_ROWS - 1) / QUANT_ROWS; }

int launch_quant_td(cpp_ctx* ctx, const float* theta, const float* ttheta, const float* r, const float* mask, float discount, int B, int N,
                    float kappa, int drop_top, float* q_out, float* tq_out, float* theta_out, float* sorted_out, float* y_out, float* td,
                    float* dz, double* loss_part, const float* w) {
  if (B < 1 || N < 2 || N > 64 || drop_top < 0 || drop_top > N - 1 || !(kappa > 0.f) || quant_td_grid(B) > DDPG_HEADS_MAX_WGS) {
    cpp_set_error("launch_quant_td: B %d, N %d, drop %d, kappa %g", B, N, drop_top, (double)kappa);
    return 1;
  }
  QuantTdArgs a;
  a.theta = theta; a.ttheta = ttheta; a.r = r; a.mask = mask; a.w = w;
  a.discount = discount; a.kappa = kappa;
  a.B = B; a.N = N; a.M = N - drop_top;
  a.q_out = q_out; a.tq_out = tq_out; a.theta_out = theta_out; a.sorted_out = sorted_out; a.y_out = y_out; a.td = td; a.dz = dz;
  a.loss_part = loss_part;
  prof_begin(ctx);
  if (w) hipLaunchKernelGGL(quant_td_weighted_kernel, dim3(quant_td_grid(B)), dim3(64 * QUANT_ROWS), 0, ctx->stream, a);
  else hipLaunchKernelGGL(quant_td_kernel, dim3(quant_td_grid(B)), dim3(64 * QUANT_ROWS), 0, ctx->stream, a);
  LAUNCH_CHECK();
  prof_end(ctx, K_QUANT);
  return 0;
}
