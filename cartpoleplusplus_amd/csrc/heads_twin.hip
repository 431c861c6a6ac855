// The DDPG heads kernel for twin Q heads (TD3's clipped double-Q on a shared representation: rt_net.cpp, cpp_net_create_twin_q): the 24 instances
// of heads_body.h with HEADS_TWIN defined, in a translation unit of their own.  A twin instance stages [W3b; b3b], its target, wqb and its target
// in LDS behind the plain layout (the same batched load block: every global load is issued before the first use), carries head 2 on the fed
// action and head 2 of the target through the concat loop, takes the smaller of the two target team sums, and leaves h3b, dz3b, Q2, Q2', td_2 and
// dz_q2; the shared layer's dz is (head 1's term) + (head 2's), then the mask; the loss partial is the sum of w (td_1^2 + td_2^2).
#define HEADS_TWIN 1
#define HEADS_KERNEL ddpg_heads_twin_kernel
#include "heads_body.h"
#undef HEADS_KERNEL

int launch_ddpg_heads_twin(cpp_ctx* ctx, const DdpgHeadsArgs& h, size_t lds) {
  typedef void (*kern_t)(const DdpgHeadsArgs);
#define HEADS_SIX(W, S) ddpg_heads_twin_kernel<1, true, W, S>, ddpg_heads_twin_kernel<2, true, W, S>, ddpg_heads_twin_kernel<4, true, W, S>, \
                        ddpg_heads_twin_kernel<8, true, W, S>, ddpg_heads_twin_kernel<4, false, W, S>, ddpg_heads_twin_kernel<8, false, W, S>
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
