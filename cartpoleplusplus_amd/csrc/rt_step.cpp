// What the DDPG and the NAF learner share of a training call: the minibatch loop of the fused inner step with its riders, the
// next-minibatch descriptor of the optimiser's launch, the route check of the entry points and the readbacks of the accessors
#include <utility>
#include "rt_internal.h"

GemmArgs sq_gemm(cpp_ctx* ctx, int list, GemmArgs g) {
  const int tiles = gemm_tiles(g.M, g.N, g.K);
  if (ctx->sq_n[list] >= 0 && ctx->sq_n[list] + tiles <= SQ_REGION) { g.sq_part = ctx->sq_part + list * SQ_REGION + ctx->sq_n[list]; ctx->sq_n[list] += tiles; }
  else ctx->sq_n[list] = -1;
  return g;
}

double* sq_take(cpp_ctx* ctx, int list, int count) {
  if (ctx->sq_n[list] < 0) return nullptr;
  if (ctx->sq_n[list] + count > SQ_REGION) { ctx->sq_n[list] = -1; return nullptr; }
  double* p = ctx->sq_part + list * SQ_REGION + ctx->sq_n[list];
  ctx->sq_n[list] += count;
  return p;
}

StatsRide next_stats_ride(cpp_ctx* ctx, const NextBatch& nx) {
  StatsRide sr;
  sr.part = nx.b->part; sr.white = nx.b->white; sr.nparts = nx.B; sr.jobs = 2 * nx.C; sr.C = nx.C;
  sr.count = (double)nx.B * (double)(nx.elems / nx.C); sr.eps = 1e-6; sr.wmax = ctx->white_max_dev;
  return sr;
}
void opt_next_stats(cpp_ctx* ctx, OptSegs& s, const NextBatch& nx) {
  if (!nx.b || nx.C <= 0 || nx.tables_done) return;
  const StatsRide sr = next_stats_ride(ctx, nx);
  s.st_part = sr.part; s.st_white = sr.white; s.st_nparts = sr.nparts; s.st_jobs = sr.jobs; s.st_C = sr.C;
  s.st_count = sr.count; s.st_eps = sr.eps; s.st_wmax = sr.wmax;
}
bool opt_closing_riders(cpp_ctx* ctx, OptSegs& s, const OptPlan& p, std::initializer_list<cpp_net*> targets, float coeff) {
  const bool last = !p.next.b;
  const bool ride = p.closes_step && last && p.actor && p.critic;
  if (ride) {
    int k = 0;
    for (cpp_net* t : targets) { s.tgt[k++] = t->params; t->wimg_key = nullptr; }
    s.tgt_coeff = coeff;
  }
  if (p.closes_call && last && ctx->route_pin_dev) { s.pub_wmax = ctx->white_max_dev; s.pub_tag = ctx->route_tag_dev; s.pub_pin = ctx->route_pin_dev; }
  return ride;
}
int opt_norms(cpp_ctx* ctx, OptSegs& s, const OptPlan& p, int lists, double* norm_part) {
  bool fold = p.folded && p.actor && p.critic && p.grad_scale == 1.0f;
  for (int l = 0; l < lists; ++l) fold = fold && p.pass.sq_cnt[l] > 0;
  if (!fold) return launch_sumsq(ctx, s, p.grad_scale, norm_part, NORM_PARTS);
  s.sq = ctx->sq_part;
  for (int l = 0; l < lists; ++l) { s.sq_begin[l] = l * SQ_REGION; s.sq_count[l] = p.pass.sq_cnt[l]; }
  return CPP_OK;
}

// conv1's weights and biases open the flat buffer (cpp_net_var_info order): [w_off, b_off + nout)
bool conv1_opens_params(const cpp_net* n) {
  const ConvL& L = n->conv[0];
  return L.w_off == 0 && L.b_off == (long)L.ks * L.ks * L.Cin * kConvOut;
}
void opt_img_net(OptSegs& s, int j, cpp_net* n, int seg, int col, const NextBatch& nx) {
  const ConvL& L = n->conv[0];
  s.img[j].w = n->params + L.w_off; s.img[j].bias = n->params + L.b_off;
  if (seg >= 0) { s.img_skip[seg] = L.b_off + kConvOut; s.img[j].gw = s.g[seg] + L.w_off; s.img[j].gb = s.g[seg] + L.b_off; }
  s.img[j].rec = reinterpret_cast<unsigned char*>(n->wimg); s.img[j].seg = seg >= 0 ? seg : 0; s.img[j].col = col; s.img[j].nout = kConvOut;
  s.img[j].white = nx.tables_done ? nx.b->white + (long)col * 2 * nx.C : nullptr;
}
void opt_img_built(const OptSegs& s, cpp_net* const* nets, const NextBatch& nx) {
  for (int j = 0; j < s.img_n; ++j) nets[j]->wimg_key = nx.b->white + (long)s.img[j].col * 2 * nx.C;
}

int step_allreduce(cpp_ctx* ctx, cpp_comm* comm, float* grads, size_t n) {
  if (!comm) return CPP_OK;
  prof_begin(ctx);
  NCCL_CHECK(ncclAllReduce(grads, grads, n, ncclFloat, ncclSum, comm->comm, ctx->stream));
  prof_end(ctx, K_ALLREDUCE);
  return CPP_OK;
}

bool route_check(cpp_ctx* ctx, uint64_t* epoch, uint64_t* gen, std::initializer_list<cpp_net*> nets) {
  ctx_route_update(ctx);
  if (*epoch == ctx->kernel_epoch) return false;
  *epoch = ctx->kernel_epoch;
  ++*gen;
  for (cpp_net* n : nets) n->wimg_key = nullptr;
  return true;
}

int read_back(cpp_ctx* ctx, std::initializer_list<Readback> items, bool through_ctx) {
  for (const Readback& i : items)
    if (i.dst) HIP_CHECK(hipMemcpyAsync(i.dst, i.src, i.bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (through_ctx) HIP_CHECK(ctx_sync_stream(ctx));
  else HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return CPP_OK;
}

// n_batches minibatches of the inner step (ddpg_cartpole.py:331-334, naf_cartpole.py:367-371) on the learner's step_batch.
// The sample + statistics pass of minibatch i + 1 depends on nothing minibatch i computes: it rides in the launch of i's conv1 dW (the
// slots double-buffered: direct replay, conv1_dw_gather.hip) or of its dW reductions (reduce_gather_kernel, replay.hip), keyed by the
// sampler's counter + 1 -- the counter itself moves in i's optimiser launch, so the rows drawn are the same.  Conv trunks on f16 / u8
// stores; CPP_RIDE_GATHER=0: in sequence.  When it leaves with conv1's dW its whitening tables are finished in the dW reductions' launch
// (flush_dw_reduce): they are in memory before the optimiser's launch, whose conv1 image rider reads them; otherwise that launch
// finishes them.
// Prioritized memory (per.hip): minibatch i's rows are the caller's or a stratified draw by priority, keyed by the sampler's counter as
// the uniform draw is; its importance weights scale the loss.  As soon as its TD values are known, ONE launch (PerPass::hook: the gradient pass
// places it behind its TD kernel) writes its priorities into the tree and draws minibatch i + 1 -- before the pass that gathers i + 1,
// wherever that rides.  The gathers take the drawn rows as a row list.  Who moves the counter then: the optimiser's launch as before
// (the draw looks one ahead: counter_add), or -- draws_bump, for a learner whose optimiser launch can stand down -- the draws themselves.
// What follows the last minibatch (target updates, the route's publish) is the learner's.
int run_minibatches(const MinibatchLoop& L, int B, int n_batches, const int32_t* rows_dev, uint64_t seed) {
  cpp_ctx* ctx = L.ctx; cpp_replay* r = L.r; cpp_batch* sb = L.step_batch;
  const int C = L.trunk->spec.pixel ? L.trunk->spec.C : 0;
  const bool direct = direct_replay_ok(L.trunk, r, B);
  static const bool no_ride = cpp_switch_off("CPP_RIDE_GATHER");
  static const bool no_dwride = cpp_switch_off("CPP_RIDE_DW");
  static const bool no_stats_ride = cpp_switch_off("CPP_RIDE_STATS");
  const bool ride_ok = !no_ride && C > 0 && L.ride_ok && (r->store_dtype == CPP_F16 || r->store_dtype == CPP_U8);
  const bool per = r->per_tree != nullptr;
  auto rows_of = [&](int i) -> const int32_t* { return rows_dev ? rows_dev + (size_t)i * B : per ? r->per_rows : nullptr; };
  auto sample = [&](int i) { return replay_sample_device(r, B, rows_of(i), seed, rows_of(i) ? nullptr : r->counter, C, sb, direct); };
  auto per_draw = [&](PerArgs& p, int i, int ahead) {       // minibatch i's rows (unless the caller's) and weights
    p.B = B; p.w_rows = rows_dev ? rows_of(i) : nullptr; p.seed = seed; p.counter = rows_dev ? nullptr : r->counter;
    if (L.draws_bump) p.bump = rows_dev ? 0 : 1;
    else p.counter_add = ahead;
    p.out_rows = r->per_rows; p.out_w = r->per_w;
  };
  PerPass pp;
  if (per) {
    pp.w = r->per_w;
    PerArgs p = per_args(r);
    per_draw(p, 0, 0);
    RC(launch_per_update_sample(ctx, p));
  }
  RC(sample(0));
  for (int i = 0; i < n_batches; ++i) {
    GatherArgs ga; StatsRide sr; int Cg = 0;
    const bool more = i + 1 < n_batches;
    if (per) {
      PerArgs p = per_args(r);
      p.up_rows = rows_of(i); p.n_up = B; p.up_td = L.td; p.skip_if_set = L.skip_if_set;
      if (more) per_draw(p, i + 1, 1);
      pp.hook = [ctx, p] { return launch_per_update_sample(ctx, p); };
    }
    bool rode, tables_done; int rc; PassLeft left;
    {
      RideScope ride(ctx);
      if (more && ride_ok) {
        ga = replay_gather_args(r, B, rows_of(i + 1), seed, rows_of(i + 1) ? nullptr : r->counter, C, sb, direct, &Cg);
        ga.counter_add = 1;
        ride.arm(&ga, sb, r->store_dtype, direct, direct && !no_dwride);
      }
      if (ctx->ride && ctx->ride_at_dw && Cg > 0 && !no_stats_ride) {
        sr = next_stats_ride(ctx, NextBatch{sb, B, Cg, r->elems, false});
        ride.arm_stats(&sr);
      }
      rc = L.gradients(pp, &left);
      rode = ride.rode(); tables_done = ride.tables_done();
    }
    if (rode && direct) { std::swap(sb->slot[0], sb->slot_alt[0]); std::swap(sb->slot[1], sb->slot_alt[1]); }
    RC(rc);
    // (the optimiser's launch also finishes the statistics of a sample pass that rode along above, unless the dW reductions' launch has)
    const bool stats_ride = rode && Cg > 0 && !(L.stats_switch && no_stats_ride);
    RC(L.apply(more, stats_ride ? NextBatch{sb, B, Cg, r->elems, tables_done} : NextBatch{}, left));
    if (more) {
      if (stats_ride) { sb->B = B; sb->dtype = CPP_F16; sb->stats_C = Cg; }     // (replay_sample_finish's bookkeeping)
      else if (rode) RC(replay_sample_finish(r, B, Cg, C, sb));
      else RC(sample(i + 1));
    }
  }
  return CPP_OK;
}
