// Prioritized experience replay (Schaul et al. 2016, proportional variant) on the device: the sum tree of the row priorities, the
// stratified draw and the importance weights (semantics: include/cartpolepp_abi.h, DESIGN "Prioritized replay").
//
// The tree is complete, in f64, heap layout: node 1 is the root, leaf i sits at node 2^L + i (2^L >= buffer_size) and holds
// (double)p_i; every inner node is left + right of its final children, so the tree does not depend on the order threads run in.
//
// per_update_sample_kernel: ONE workgroup per launch, four phases:
//   (phases 1-2 stand down while the optional flag skip_if_set is non-zero: NAF's check_numerics flag keeps a non-finite minibatch out)
//   1. leaf writes of up to PER_MAX_ROWS rows (a row listed twice takes its LAST occurrence: an O(n^2) scan of the list in LDS) and
//      the running maximum priority;
//   2. the ancestors of the touched leaves, level by level, a barrier between levels (the top 10 levels in LDS);
//   3. optionally, the stratified draw of B rows (the top levels of the tree staged in LDS), or the rows of a given list;
//   4. their importance weights, normalised by the batch maximum.
// Bulk writes (enable, synthetic fill) rebuild the whole tree instead: per_leaves_kernel + one per_level_kernel per level.
#include "common.h"

constexpr int PER_TOP_LEVELS = 10;     // the ancestor updates run the tree's top levels in LDS: nodes [1, 2^10 = PER_TOP_NODES)

__device__ __forceinline__ float per_priority(float td, float alpha, float eps) {
  if (alpha == 0.f) return 1.f;
  const float x = fabsf(td) + eps;
  return alpha == 1.f ? x : powf(x, alpha);
}

// max over the workgroup (exact in any order): the waves' shuffles, then the PER_THREADS / 64 wave results; every thread gets it
template <typename T>
__device__ __forceinline__ T per_block_max(T v, T* red) {
  for (int o = 32; o > 0; o >>= 1) {
    const T x = __shfl_xor(v, o);      // (every lane shuffles, then selects: a shuffle inside the select would read inactive lanes)
    v = v > x ? v : x;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T m = red[0];
  for (int i = 1; i < PER_THREADS / 64; ++i) m = m > red[i] ? m : red[i];
  return m;
}

__global__ __launch_bounds__(PER_THREADS) void per_update_sample_kernel(const PerArgs a) {
  __shared__ int32_t rows[PER_MAX_ROWS];
  __shared__ double top[2 * PER_TOP_NODES];
  __shared__ double wv[PER_MAX_ROWS];
  __shared__ double dred[PER_THREADS / 64];
  __shared__ float fred[PER_THREADS / 64];
  const int tid = threadIdx.x, L = a.L;
  const long nleaf = 1L << L;
  double* tree = a.tree;
  if (a.n_up > 0 && !(a.skip_if_set && *a.skip_if_set)) {      // (uniform: every lane reads the same word)
    // ---- 1. leaves (+ running maximum)
    for (int b = tid; b < a.n_up; b += PER_THREADS) rows[b] = a.up_rows[b];
    const float pmax0 = *a.maxp;
    __syncthreads();
    float m = 0.f;
    for (int b = tid; b < a.n_up; b += PER_THREADS) {
      const float p = a.up_td ? per_priority(a.up_td[b], a.alpha, a.eps) : pmax0;
      m = fmaxf(m, p);
      const int row = rows[b];
      bool last = true;
      if (a.up_td)             // (new rows all take the same value: whichever occurrence lands is the last one's)
        for (int c = 0; c < a.n_up; ++c)      // (no early exit: the LDS reads of the scan pipeline, and every lane reads the same word)
          last = last && !(c > b && rows[c] == row);
      if (last) tree[nleaf + row] = (double)p;
    }
    const float mm = per_block_max(m, fred);
    if (tid == 0) *a.maxp = fmaxf(pmax0, mm);
    // ---- 2. ancestors, one level per pass (two rows under one parent write the same sum).  Levels below the top TL ones in global
    // memory; the top ones (nodes [1, 2^TL)) in LDS, with their children staged first and the result written back: a level in global
    // memory is a dependent store + load round trip, in LDS a fraction of one.
    const int TL = L < PER_TOP_LEVELS ? L : PER_TOP_LEVELS;
    for (int k = 1; k <= L - TL; ++k) {
      __syncthreads();
      for (int b = tid; b < a.n_up; b += PER_THREADS) {
        const long node = (nleaf + rows[b]) >> k;
        tree[node] = tree[2 * node] + tree[2 * node + 1];
      }
    }
    __syncthreads();
    for (long i = 1 + tid; i < (2L << TL); i += PER_THREADS) top[i] = tree[i];
    __syncthreads();
    for (int k = L - TL + 1; k <= L; ++k) {
      for (int b = tid; b < a.n_up; b += PER_THREADS) {
        const long node = (nleaf + rows[b]) >> k;
        top[node] = top[2 * node] + top[2 * node + 1];
      }
      __syncthreads();
    }
    for (long i = 1 + tid; i < (1L << TL); i += PER_THREADS) tree[i] = top[i];
    __syncthreads();
  }
  if (a.B <= 0) return;
  // ---- 3. the rows: stratified draw (Philox word 1 = 1: disjoint from the uniform sampler's stream) or the given list
  const int size = *a.size_ptr;
  const double total = tree[1];
  const long ntop = (2 * nleaf) < PER_TOP_NODES ? 2 * nleaf : PER_TOP_NODES;
  for (long i = 1 + tid; i < ntop; i += PER_THREADS) top[i] = tree[i];
  const uint64_t ctr = a.counter ? *a.counter + (uint64_t)a.counter_add : 0;
  __syncthreads();
  double wm = 0.0;
  const double nb = -(double)*a.beta;
  for (int b = tid; b < a.B; b += PER_THREADS) {
    int row;
    if (a.w_rows) {
      row = a.w_rows[b];
    } else {
      const u32x4 c = {(uint32_t)b, 1u, (uint32_t)ctr, (uint32_t)(ctr >> 32)};
      const u32x4 r = philox4x32_10(c, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
      const double U = (double)((((uint64_t)r.x << 32) | (uint64_t)r.y) >> 11) * 0x1p-53;
      double u = ((double)b + U) * (total / (double)a.B);
      long node = 1;
      for (int k = 0; k < L; ++k) {
        const long l = 2 * node;
        const double left = l < ntop ? top[l] : tree[l];
        if (u < left) node = l;
        else { u -= left; node = l + 1; }
      }
      row = (int)(node - nleaf);
      if (row >= size) row = size - 1;      // rounding at the top end walked past the last row: the last row
      a.out_rows[b] = row;
    }
    // ---- 4. importance weight (size * P(row))^-beta, P = leaf / total
    const double w = pow((double)size * tree[nleaf + row] / total, nb);
    wv[b] = w;
    wm = fmax(wm, w);
  }
  const double wmax = per_block_max(wm, dred);
  if (a.bump && tid == 0) *a.counter += 1;      // (every thread has read the counter: the barrier in per_block_max)
  for (int b = tid; b < a.B; b += PER_THREADS) a.out_w[b] = (float)(wv[b] / wmax);
}

int launch_per_update_sample(cpp_ctx* ctx, const PerArgs& a) {
  prof_begin(ctx);
  hipLaunchKernelGGL(per_update_sample_kernel, dim3(1), dim3(PER_THREADS), 0, ctx->stream, a);
  LAUNCH_CHECK();
  prof_end(ctx, K_PER);
  return 0;
}

// leaf i = i < n ? *maxp : 0 (rows [n, 2^L) are not in the memory and are never drawn)
__global__ void per_leaves_kernel(double* tree, long nleaf, long n, const float* maxp) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nleaf) tree[nleaf + i] = i < n ? (double)*maxp : 0.0;
}

__global__ void per_level_kernel(double* tree, long first, long count) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) { const long node = first + i; tree[node] = tree[2 * node] + tree[2 * node + 1]; }
}

int launch_per_rebuild(cpp_ctx* ctx, double* tree, int L, long n, const float* maxp) {
  const long nleaf = 1L << L;
  prof_begin(ctx);
  hipLaunchKernelGGL(per_leaves_kernel, dim3((unsigned)((nleaf + 255) / 256)), dim3(256), 0, ctx->stream, tree, nleaf, n, maxp);
  LAUNCH_CHECK();
  for (int k = L - 1; k >= 0; --k) {
    const long count = 1L << k;
    hipLaunchKernelGGL(per_level_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, tree, count, count);
    LAUNCH_CHECK();
  }
  prof_end(ctx, K_PER);
  return 0;
}
