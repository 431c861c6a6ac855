// DDPG "heads" kernel: everything between the last hidden layers of the four networks and the first backward GEMMs,
// row-local work that would otherwise be five dependent GEMM levels of a few thousand multiply-adds per row.
//
// Per batch row (ddpg_cartpole.py:95-100, :111-113, :166-171, :180-184, :199-209, :222):
//   a   = tanh(h2a Wo + bo)                               actor head            a' likewise from the target actor
//   h3  = relu([h2c, a] W3 + b3),  dQ/da at a = mu(s1)     critic, 2nd evaluation -> actor's grad_ys = -dQ/da through tanh
//   q   = relu([h2c, a_batch] W3 + b3) wq + bq             critic on the fed actions
//   q'  = relu([h2c', a'] W3' + b3') wq' + bq'              target critic at the target actor's action
//   td  = q - (r + mask discount q'),  loss = mean(td^2),  dz_q = 2 td / B   (prioritized replay: mean(w td^2), 2 td w / B)
//   and one layer of both backward passes: dz of the critic's concat layer and of the layers feeding the two heads.
// A team of 64 lanes (one wave) works on one row, a workgroup of 256 threads on 4 rows (grid = B / 4); the weights it needs sit
// in LDS (lane t owns unit t of the concat layer and element t of every row vector).  The batch loss is
// left as one partial per workgroup; whoever reads the loss adds them in order.
#define HEADS_KERNEL ddpg_heads_kernel
#include "heads_body.h"
#undef HEADS_KERNEL

int launch_ddpg_heads_twin(cpp_ctx* ctx, const DdpgHeadsArgs& h, size_t lds);      // heads_twin.hip
int launch_ddpg_heads_twin_min(cpp_ctx* ctx, const DdpgHeadsArgs& h, size_t lds);  // heads_twin_min.hip

size_t ddpg_heads_lds_bytes(const DdpgHeadsArgs& h) {
  const size_t k3 = h.n2c + h.A + 1, n3p = HEADS_N3P, n2cp = (h.n2c + 3) & ~3;
  const size_t wfl = (k3 * h.n3 + HEADS_WSLACK + 3) & ~(size_t)3;
  const size_t n1ap = (h.n1a + 3) & ~3, w2fl = h.n1a ? (((n1ap + 1) * h.n2a + HEADS_WSLACK + 3) & ~(size_t)3) : 0;
  const size_t w = ((2 * wfl + 2 * (n3p + 4) + 2 * (size_t)(h.n2a + 1) * h.A + 3) & ~(size_t)3) + 2 * w2fl;
  size_t f = w + (size_t)HEADS_ROWS * (n3p + 2 * n2cp + ((2 * h.n2a + 3) & ~3) + (h.n1a ? HEADS_TEAM + 2 * n1ap : 0));
  if (h.W3b) f += 2 * wfl + 2 * (n3p + 4) + (size_t)HEADS_ROWS * n3p;      // twin Q heads: two more images, a second dz3 row per team
  return f * sizeof(float);
}

bool ddpg_heads_supported(const DdpgHeadsArgs& h) {
  if (h.n1a && !(h.n1a <= HEADS_N1MAX && (h.n2a & 1) == 0 &&
                 (((h.n1a + 3) & ~3) + 1) * h.n2a + HEADS_WSLACK + 4 <= 4 * HEADS_NW4P * HEADS_THREADS)) return false;
  return h.A <= HEADS_AMAX && h.n3 <= HEADS_N3P && h.n2a <= HEADS_TEAM && h.n2c <= HEADS_TEAM &&
         (h.n2a + 1) * h.A <= 2 * HEADS_THREADS && (h.n2c + h.A + 1) * h.n3 + HEADS_WSLACK + 4 <= 4 * HEADS_NW4 * HEADS_THREADS && (h.n3 & 1) == 0 && ddpg_heads_lds_bytes(h) <= 120 * 1024 && (h.B + HEADS_ROWS - 1) / HEADS_ROWS <= DDPG_HEADS_MAX_WGS;
}

int launch_ddpg_heads(cpp_ctx* ctx, const DdpgHeadsArgs& h) {
  const size_t lds = ddpg_heads_lds_bytes(h);
  typedef void (*kern_t)(const DdpgHeadsArgs);
  if (h.min_sel) return launch_ddpg_heads_twin_min(ctx, h, lds);      // (twin Q heads, the actor on the smaller head: heads_twin_min.hip)
  if (h.W3b) return launch_ddpg_heads_twin(ctx, h, lds);      // (twin Q heads: the instances of heads_twin.hip)
#define HEADS_SIX(W, S) ddpg_heads_kernel<1, true, W, S>, ddpg_heads_kernel<2, true, W, S>, ddpg_heads_kernel<4, true, W, S>, \
                        ddpg_heads_kernel<8, true, W, S>, ddpg_heads_kernel<4, false, W, S>, ddpg_heads_kernel<8, false, W, S>
  static const kern_t kerns[24] = {HEADS_SIX(false, false), HEADS_SIX(true, false), HEADS_SIX(false, true), HEADS_SIX(true, true)};
#undef HEADS_SIX
  const int ki = (h.A == 1 ? 0 : h.A == 2 ? 1 : h.A == 4 ? 2 : h.A == 8 ? 3 : h.A == 3 ? 4 : 5) + (h.w ? 6 : 0) + (h.tps.n ? 12 : 0);
  static size_t attr[CPP_MAX_DEVICES][24] = {};      // (kernel attributes are per device)
  size_t& have = attr[cpp_dev_slot(ctx)][ki];
  if (lds > have) {
    HIP_CHECK(hipFuncSetAttribute((const void*)kerns[ki], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    have = lds;
  }
  prof_begin(ctx);
  hipLaunchKernelGGL(kerns[ki], dim3((h.B + HEADS_ROWS - 1) / HEADS_ROWS), dim3(HEADS_THREADS), lds, ctx->stream, h);
  LAUNCH_CHECK();
  prof_end(ctx, K_HEADS);
  return 0;
}

// ---- target policy smoothing where the heads kernel does not run (GEMM levels: A > 8, wide or low-dimensional stacks; the single
// train ops): the same function over the B x A action columns the target critic is about to read
__global__ __launch_bounds__(256) void tps_smooth_kernel(const TpsArgs s, const float* __restrict__ in, int ld_in, float* out, int ld_out, int B, int A) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= B * A) return;
  const unsigned long long n = s.n[0];                 // (read only, as in the heads kernel)
  const int b = i / A, c = i - b * A;
  const float e = tps_noise(s, n, (unsigned)b, (unsigned)c);
  s.eps[i] = e;
  out[(long)b * ld_out + c] = tps_apply(in[(long)b * ld_in + c], e);
  if (i == 0) s.n_out[0] = n;
}

int launch_tps_smooth(cpp_ctx* ctx, const TpsArgs& s, const float* in, int ld_in, float* out, int ld_out, int B, int A) {
  prof_begin(ctx);
  hipLaunchKernelGGL(tps_smooth_kernel, dim3((B * A + 255) / 256), dim3(256), 0, ctx->stream, s, in, ld_in, out, ld_out, B, A);
  LAUNCH_CHECK();
  prof_end(ctx, K_ELEMENTWISE);
  return 0;
}

// ---- delayed policy updates where the heads kernel does not count the minibatch (common.h: launch_pd_tick): the same arithmetic, one thread
__global__ void pd_tick_kernel(unsigned long long* pd, unsigned pd_d, unsigned long long* step, int do_actor, int do_critic, int peek) {
  const unsigned long long ph = pd[PD_PHASE] + 1ull;
  const unsigned long long act = ph == (unsigned long long)pd_d ? 1ull : 0ull;
  pd[PD_HOLD] = 1ull - act;
  if (!peek) { pd[PD_N] += 1ull; pd[PD_PHASE] = act ? 0ull : ph; }
  if (step && do_actor) step[0] += act;
  if (step && do_critic) step[1] += 1ull;
}

int launch_pd_tick(cpp_ctx* ctx, uint64_t* pd, unsigned pd_d, uint64_t* step, bool do_actor, bool do_critic, bool peek) {
  prof_begin(ctx);
  hipLaunchKernelGGL(pd_tick_kernel, dim3(1), dim3(1), 0, ctx->stream, (unsigned long long*)pd, pd_d, (unsigned long long*)step, do_actor ? 1 : 0, do_critic ? 1 : 0, peek ? 1 : 0);
  LAUNCH_CHECK();
  prof_end(ctx, K_ELEMENTWISE);
  return 0;
}
