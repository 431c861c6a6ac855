// The DDPG heads kernel for twin Q heads whose actor follows the smaller online head (cpp_ddpg_set_actor_min_q): the 24 instances of
// heads_body.h with HEADS_TWIN and HEADS_TWIN_MIN defined, in a translation unit of their own -- the plain and the twin instances keep their
// token streams.  On top of a twin instance: head 2's concat sum at a = mu(s1) (one more accumulator through the action loop), Q1 and Q2 there
// (two more team sums), the row's choice (wave-uniform; a tie is head 1's), and dz of the concat layer and dQ/da from the chosen head's wq and
// [W3; b3] action rows, all of which the twin instance holds in LDS already.  Three more stores per row: Q1, Q2 and the choice.
#define HEADS_TWIN 1
#define HEADS_TWIN_MIN 1
#define HEADS_KERNEL ddpg_heads_twin_min_kernel
#include "heads_body.h"
#undef HEADS_KERNEL

int launch_ddpg_heads_twin_min(cpp_ctx* ctx, const DdpgHeadsArgs& h, size_t lds) {
  typedef void (*kern_t)(const DdpgHeadsArgs);
#define HEADS_SIX(W, S) ddpg_heads_twin_min_kernel<1, true, W, S>, ddpg_heads_twin_min_kernel<2, true, W, S>, ddpg_heads_twin_min_kernel<4, true, W, S>, \
                        ddpg_heads_twin_min_kernel<8, true, W, S>, ddpg_heads_twin_min_kernel<4, false, W, S>, ddpg_heads_twin_min_kernel<8, false, W, S>
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
