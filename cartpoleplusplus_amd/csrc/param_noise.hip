// Parameter-space exploration noise (Plappert et al. 2018; cpp_ddpg_set_param_noise / cpp_ddpg_param_noise_resample; an extension of the
// exploration of ddpg_cartpole.py:127-134, whose Ornstein-Uhlenbeck sample is added to the action on the host).  Two launches per resample,
// both reading the trainer's words (common.h: PnWords) from device memory, so that the host waits for nothing:
//   pn_perturb_kernel   the perturbed copy pt[i] = fmaf(sigma, z(seed, n, i), p[i]) of the actor's flat parameter buffer; the feature layer
//                       norm's gamma and beta, which close the buffer, are copied.  Memory-bound by its traffic (8 bytes per element) but
//                       ten Philox rounds, a logf and a cospif per element: the grid is sized to fill the chip and strides the rest.  The
//                       Philox counter is the ELEMENT index, so the result does not depend on the grid, the block or the vector width.
//                       128-bit loads and stores (plain C++ vector accesses: no buffer store, nothing for the store checker) where both
//                       pointers are 16-byte aligned, a scalar tail (and a scalar body where they are not).
//   pn_measure_kernel   one workgroup: the distance between the two action batches in f64 in one fixed order (bc.hip's pattern), the
//                       adapted sigma for the NEXT resample, the count.  It alone writes the words.
#include "common.h"

__device__ __forceinline__ float pn_value(float p, float sigma, unsigned seed_lo, unsigned seed_hi, unsigned long long n, long i, long n_noise) {
  return i < n_noise ? __builtin_fmaf(sigma, pn_normal(seed_lo, seed_hi, n, (unsigned)i), p) : p;
}

__global__ __launch_bounds__(PN_THREADS) void pn_perturb_kernel(const PnWords* __restrict__ words, unsigned seed_lo, unsigned seed_hi,
                                                                const float* __restrict__ src, float* __restrict__ dst, long count, long n_noise,
                                                                int vec_ok) {
  const float sigma = words->sigma;
  const unsigned long long n = words->n;
  const long tid = (long)blockIdx.x * PN_THREADS + threadIdx.x, stride = (long)gridDim.x * PN_THREADS;
  const long nvec = vec_ok ? count / 4 : 0;
  for (long v = tid; v < nvec; v += stride) {
    const f32x4 p = *reinterpret_cast<const f32x4*>(src + 4 * v);
    f32x4 o;
    o.x = pn_value(p.x, sigma, seed_lo, seed_hi, n, 4 * v + 0, n_noise);
    o.y = pn_value(p.y, sigma, seed_lo, seed_hi, n, 4 * v + 1, n_noise);
    o.z = pn_value(p.z, sigma, seed_lo, seed_hi, n, 4 * v + 2, n_noise);
    o.w = pn_value(p.w, sigma, seed_lo, seed_hi, n, 4 * v + 3, n_noise);
    *reinterpret_cast<f32x4*>(dst + 4 * v) = o;
  }
  for (long i = 4 * nvec + tid; i < count; i += stride) dst[i] = pn_value(src[i], sigma, seed_lo, seed_hi, n, i, n_noise);
}

__global__ __launch_bounds__(PN_THREADS) void pn_measure_kernel(PnWords* words, const float* __restrict__ a, const float* __restrict__ at, int count,
                                                                float delta, float alpha, float* __restrict__ a_keep, float* __restrict__ at_keep) {
  __shared__ double part[PN_THREADS];
  const int t = (int)threadIdx.x;
  double acc = 0.0;
  for (int i = t; i < count; i += PN_THREADS) {
    const float x = a[i], y = at[i];
    a_keep[i] = x; at_keep[i] = y;
    const double diff = (double)x - (double)y;      // (exact)
    acc += diff * diff;
  }
  part[t] = acc;
  __syncthreads();
  for (int w = PN_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) part[t] += part[t + w];
    __syncthreads();
  }
  if (t != 0) return;
  PnWords w = *words;
  if (count > 0) {
    w.d = (float)sqrt(part[0] / (double)count);
    w.sigma = w.d < delta ? w.sigma * alpha : w.sigma / alpha;      // (read by the next resample's first launch)
    w.adapted = 1u;
  } else {
    w.adapted = 0u;
  }
  w.n += 1ull;
  *words = w;
}

int launch_pn_perturb(cpp_ctx* ctx, const PnWords* words, uint64_t seed, const float* src, float* dst, long count, long n_noise) {
  if (!words || !src || !dst || src == dst || count < 1 || count > 0xFFFFFFFFl || n_noise < 0 || n_noise > count) {
    cpp_set_error("launch_pn_perturb: %ld elements, %ld perturbed", count, n_noise);
    return 1;
  }
  const int vec_ok = (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0;
  long blocks = (count / 4 + PN_THREADS - 1) / PN_THREADS;
  const long cap = (long)ctx->num_cus * 8;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  prof_begin(ctx);
  hipLaunchKernelGGL(pn_perturb_kernel, dim3((unsigned)blocks), dim3(PN_THREADS), 0, ctx->stream, words, (unsigned)seed, (unsigned)(seed >> 32), src, dst,
                     count, n_noise, vec_ok);
  LAUNCH_CHECK();
  prof_end(ctx, K_PARAM_NOISE);
  return 0;
}

int launch_pn_measure(cpp_ctx* ctx, PnWords* words, const float* a, const float* at, int B, int A, float delta, float alpha, float* a_keep, float* at_keep) {
  if (!words || B < 0 || A < 1 || (B > 0 && (!a || !at || !a_keep || !at_keep)) || (long)B * A > 0x7FFFFFFFl) {
    cpp_set_error("launch_pn_measure: B %d, A %d", B, A);
    return 1;
  }
  prof_begin(ctx);
  hipLaunchKernelGGL(pn_measure_kernel, dim3(1), dim3(PN_THREADS), 0, ctx->stream, words, a, at, B * A, delta, alpha, a_keep, at_keep);
  LAUNCH_CHECK();
  prof_end(ctx, K_PARAM_NOISE);
  return 0;
}
