// Feature layer norm: Linear -> LayerNorm -> tanh / relu on fully connected layer 0 of a pixel network (the trunk of DrQ-v2, Yarats et al.
// 2021) -- an extension of the first hidden layer of ddpg_cartpole.py:95 (actor, 'h0') and :168 (critic, 'hidden1').  The definition is
// include/cartpolepp_abi.h's (cpp_net_create_feature_norm); tests/layer_norm_np.py restates it.
//
// dist.hip's idiom: one wave per row, the rows of several networks as a job list in one launch (blockIdx.y).  A row of up to LN_MAX_WIDTH
// values is read once, lane-strided (lane l holds columns l, l + 64, ..), and stays in registers; mean and variance are two passes over the
// registers; the cross-lane sums are one fixed xor butterfly, so every lane holds the same bits.  f32 operations are rounded one by one
// (contraction off), tanhf is the accurate one.  The forward and the row-local backward use no LDS; no atomics, no scratch.
//
// Backward: the column sums dgamma / dbeta run over the batch in an order that is a function of B alone, never of the grid -- sixteen
// contiguous parts of the batch, each with b ascending, added in order (8 KB of LDS) --, in a launch of their own in front of the
// row-local kernel that turns g = dL/dy into dL/dz in place.  Each column workgroup leaves the f64 sum of squares of the gradients it
// wrote in its own slot of the list's squared-norm partials (cpp_ctx::sq_part).
#include "common.h"

#pragma clang fp contract(off)

constexpr int LN_ROWS = 4;                        // rows (waves) per workgroup
constexpr int LN_PER_LANE = LN_MAX_WIDTH / 64;    // values of a row a lane holds
constexpr int LN_SEGS = 16;                       // the column sums' waves per workgroup: contiguous sixteenths of the batch

__device__ __forceinline__ float ln_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double ln_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
  return v;
}
// act'(y) from the layer's own output: 1 - y^2, or y > 0
__device__ __forceinline__ float ln_act_grad(float y, int act) { return act == GE_TANH ? 1.f - y * y : (y > 0.f ? 1.f : 0.f); }

__global__ __launch_bounds__(64 * LN_ROWS) void ln_forward_kernel(LnArgs a) {
  const LnJob& j = a.j[blockIdx.y];
  const int lane = threadIdx.x & 63, b = blockIdx.x * LN_ROWS + (threadIdx.x >> 6);
  if (b >= a.B) return;      // (wave-uniform)
  const int n = j.n;
  float* row = j.io + (long)b * j.ld;
  float v[LN_PER_LANE];
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < LN_PER_LANE; ++k) {
    const int c = lane + 64 * k;
    v[k] = c < n ? row[c] : 0.f;
    s = s + v[k];
  }
  const float mu = ln_wave_sum(s) / (float)n;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < LN_PER_LANE; ++k) {
    const int c = lane + 64 * k;
    v[k] = c < n ? v[k] - mu : 0.f;
    q = q + v[k] * v[k];
  }
  const float var = ln_wave_sum(q) / (float)n;
  const float rstd = 1.f / sqrtf(var + a.eps);
#pragma unroll
  for (int k = 0; k < LN_PER_LANE; ++k) {
    const int c = lane + 64 * k;
    if (c < n) {
      const float xh = v[k] * rstd;
      const float u = j.gamma[c] * xh + j.beta[c];
      row[c] = a.act == GE_TANH ? tanhf(u) : fmaxf(u, 0.f);
      j.xhat[(long)b * n + c] = xh;
    }
  }
  if (lane == 0) j.rstd[b] = rstd;
}

// dgamma_c = sum_b du_bc xhat_bc, dbeta_c = sum_b du_bc with du = g act'(y): 64 columns per workgroup, one thread per column and
// sixteenth of the batch -- wave s adds rows [s ceil(B / 16), (s + 1) ceil(B / 16)) with b ascending, wave 0 adds the sixteen partials in
// order.  The order is a function of B alone.
__global__ __launch_bounds__(64 * LN_SEGS) void ln_backward_cols_kernel(LnArgs a) {
  __shared__ float part[2][LN_SEGS][64];
  const LnJob& j = a.j[blockIdx.y];
  const int n = j.n;
  if (blockIdx.x * 64 >= n) return;      // (uniform: a narrower network of the same launch)
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
  const int per = (a.B + LN_SEGS - 1) / LN_SEGS, b0 = seg * per, b1 = min(a.B, b0 + per);
  const float* __restrict__ g = j.dz;
  const float* __restrict__ y = j.io;
  const float* __restrict__ xh = j.xhat;
  float dg = 0.f, db = 0.f;
  if (c < n) {
#pragma unroll 4
    for (int b = b0; b < b1; ++b) {
      const float du = g[(long)b * n + c] * ln_act_grad(y[(long)b * j.ld + c], a.act);
      dg = dg + du * xh[(long)b * n + c];
      db = db + du;
    }
  }
  part[0][seg][lane] = dg;
  part[1][seg][lane] = db;
  __syncthreads();
  if (seg != 0) return;
  dg = 0.f; db = 0.f;
#pragma unroll
  for (int s = 0; s < LN_SEGS; ++s) { dg = dg + part[0][s][lane]; db = db + part[1][s][lane]; }
  if (c < n) {
    j.dgamma[c] = dg;
    j.dbeta[c] = db;
  }
  if (j.sq_part) {                       // (uniform) this workgroup's share of the gradient list's squared norm, fixed order
    const double sq = ln_wave_sum((double)dg * (double)dg + (double)db * (double)db);
    if (lane == 0) j.sq_part[blockIdx.x] = sq;
  }
}

// dz = rstd (dxh - mean_j dxh - xhat mean_j(dxh xhat)), dxh = g act'(y) gamma: row-local, in place on g
__global__ __launch_bounds__(64 * LN_ROWS) void ln_backward_rows_kernel(LnArgs a) {
  const LnJob& j = a.j[blockIdx.y];
  const int lane = threadIdx.x & 63, b = blockIdx.x * LN_ROWS + (threadIdx.x >> 6);
  if (b >= a.B) return;      // (wave-uniform)
  const int n = j.n;
  float* grow = j.dz + (long)b * n;
  const float* yrow = j.io + (long)b * j.ld;
  const float* xrow = j.xhat + (long)b * n;
  float dxh[LN_PER_LANE], xh[LN_PER_LANE];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < LN_PER_LANE; ++k) {
    const int c = lane + 64 * k;
    dxh[k] = 0.f; xh[k] = 0.f;
    if (c < n) {
      const float du = grow[c] * ln_act_grad(yrow[c], a.act);
      dxh[k] = du * j.gamma[c];
      xh[k] = xrow[c];
    }
    s1 = s1 + dxh[k];
    s2 = s2 + dxh[k] * xh[k];
  }
  const float m1 = ln_wave_sum(s1) / (float)n, m2 = ln_wave_sum(s2) / (float)n;
  const float rstd = j.rstd[b];
#pragma unroll
  for (int k = 0; k < LN_PER_LANE; ++k) {
    const int c = lane + 64 * k;
    if (c < n) grow[c] = rstd * ((dxh[k] - m1) - xh[k] * m2);
  }
}

int ln_col_blocks(int n) { return (n + 63) / 64; }

static int ln_check(const LnArgs& a, bool backward, const char* who) {
  bool ok = a.count >= 1 && a.count <= LN_JOBS_MAX && a.B >= 1 && (a.act == GE_TANH || a.act == GE_RELU) && a.eps > 0.f;
  for (int k = 0; ok && k < a.count; ++k) {
    const LnJob& j = a.j[k];
    ok = j.n >= 1 && j.n <= LN_MAX_WIDTH && j.ld >= j.n && j.io && j.gamma && j.beta && j.xhat && j.rstd;
    if (ok && backward) ok = j.dz && j.dgamma && j.dbeta;
  }
  if (!ok) { cpp_set_error("%s: %d jobs, B %d, activation %d (widths 1 .. %d, tanh or relu)", who, a.count, a.B, a.act, LN_MAX_WIDTH); return 1; }
  return 0;
}

int launch_ln_forward(cpp_ctx* ctx, const LnArgs& a) {
  if (ln_check(a, false, "launch_ln_forward")) return 1;
  prof_begin(ctx);
  hipLaunchKernelGGL(ln_forward_kernel, dim3((a.B + LN_ROWS - 1) / LN_ROWS, a.count), dim3(64 * LN_ROWS), 0, ctx->stream, a);
  LAUNCH_CHECK();
  prof_end(ctx, K_LN_FWD);
  return 0;
}

int launch_ln_backward_cols(cpp_ctx* ctx, const LnArgs& a) {
  if (ln_check(a, true, "launch_ln_backward_cols")) return 1;
  int widest = 0;
  for (int k = 0; k < a.count; ++k) widest = a.j[k].n > widest ? a.j[k].n : widest;
  prof_begin(ctx);
  hipLaunchKernelGGL(ln_backward_cols_kernel, dim3(ln_col_blocks(widest), a.count), dim3(64 * LN_SEGS), 0, ctx->stream, a);
  LAUNCH_CHECK();
  prof_end(ctx, K_LN_BWD);
  return 0;
}

int launch_ln_backward_rows(cpp_ctx* ctx, const LnArgs& a) {
  if (ln_check(a, true, "launch_ln_backward_rows")) return 1;
  prof_begin(ctx);
  hipLaunchKernelGGL(ln_backward_rows_kernel, dim3((a.B + LN_ROWS - 1) / LN_ROWS, a.count), dim3(64 * LN_ROWS), 0, ctx->stream, a);
  LAUNCH_CHECK();
  prof_end(ctx, K_LN_BWD);
  return 0;
}
