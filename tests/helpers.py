"""Shared builders for the GPU parity tests: a device agent (through the public Python surface, i.e.
through the C ABI) and an oracle agent holding the same parameters."""
import numpy as np

from oracle import ddpg_np as O


def hyper_options(hyper):
    """an O.Hyper as the command line options of ddpg_cartpole.py (make_pair's **optkw)"""
    return dict(actor_learning_rate=hyper.actor_lr, critic_learning_rate=hyper.critic_lr, discount=hyper.discount,
                gradient_clip=hyper.gradient_clip, target_update_rate=hyper.target_update_rate)


def make_opts(D, shape, B, pixel, **kw):
    if pixel:
        o = D.default_opts(use_raw_pixels=True, render_height=shape[0], render_width=shape[1],
                           num_cameras=shape[3], action_repeats=shape[4], batch_size=B, **kw)
    else:
        o = D.default_opts(use_raw_pixels=False, action_repeats=shape[0], batch_size=B, **kw)
    D.set_opts(o)
    return o


class FakeEnv(object):
    class _S(object):
        def __init__(self, shape):
            self.shape = tuple(shape)

    def __init__(self, shape, action_dim=2):
        self.observation_space, self.action_space = self._S(shape), self._S((1, action_dim))


def make_pair(shape, B, pixel, seed=0, replay_size=64, perturb=True, dt=np.float64, actor_hidden=None, critic_hidden=None,
              action_dim=2, capacity=None, **optkw):
    """returns (agent, oracle DDPG, specs).  Parameters are perturbed away from the near-zero actor
    head / zero biases so every path carries signal.  actor_hidden / critic_hidden: lists of widths
    (--actor-hidden-layers / --critic-hidden-layers; None: the defaults), action_dim: the env's action size.
    capacity: the batch size the agent is built with (--batch-size; None: B), the largest batch it takes."""
    import os
    from cartpoleplusplus_amd import ddpg_cartpole as D
    if os.environ.get("TEST_EXACT_PRODUCTS") == "1":      # (test snippets run in subprocesses: the TEST's switch for --exact-products)
        optkw.setdefault("exact_products", True)
    for key, widths in (("actor_hidden_layers", actor_hidden), ("critic_hidden_layers", critic_hidden)):
        if widths is not None:
            optkw[key] = ",".join(str(int(w)) for w in widths)
    make_opts(D, shape, B if capacity is None else int(capacity), pixel, replay_memory_size=replay_size, **optkw)
    agent = D.DeepDeterministicPolicyGradientAgent(FakeEnv(shape, action_dim))
    agent.initialise_variables(seed=seed)
    rng = np.random.default_rng(seed + 100)
    if perturb:
        for net in (agent.actor, agent.critic):
            p = net.get_params()
            net.set_params(p + rng.normal(0, 0.05, p.shape).astype(np.float32))
    agent.post_var_init_setup()
    if perturb:
        for net in (agent.target_actor, agent.target_critic):
            p = net.get_params()
            net.set_params(p + rng.normal(0, 0.01, p.shape).astype(np.float32))
    if pixel:
        kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:])), batch_norm=bool(optkw.get("use_batch_norm", False)))
    else:
        kw = dict(pixel=False, state_elems=int(np.prod(shape)))
    aspec = O.NetSpec("actor", action_dim, D._hidden(D.opts.actor_hidden_layers), dropout=bool(optkw.get("use_dropout", False)), **kw)
    cspec = O.NetSpec("critic", action_dim, D._hidden(D.opts.critic_hidden_layers), **kw)
    ref = O.DDPG(aspec, cspec, agent.actor.get_params(), agent.critic.get_params(), dt)
    ref.set_targets(agent.target_actor.get_params(), agent.target_critic.get_params())
    return agent, ref, (aspec, cspec)


def per_var_report(spec, got, want):
    """[(name, max_abs_err, rel_l2_err)] per variable of a flat vector."""
    rows, off = [], 0
    for name, shp in spec.layout():
        n = int(np.prod(shp))
        g, w = got[off:off + n].astype(np.float64), np.asarray(want[off:off + n], np.float64)
        denom = np.linalg.norm(w)
        rows.append((name, float(np.abs(g - w).max()), float(np.linalg.norm(g - w) / denom) if denom > 0 else float(np.abs(g).max())))
        off += n
    return rows


def assert_flat_close(spec, got, want, rel=2e-5, what="", abs_floor=0.0, rel_of=None):
    """abs_floor: an absolute error one-element variables are not held below (the critic's q_value bias gradient is 2 mean(td), a
    sum with cancellation: it cannot be closer to the oracle than the Q values that make up td).  rel_of: {variable: tolerance}
    that replaces `rel` where it is larger (the float32 evaluation's own distance from float64, times a factor)."""
    rows = per_var_report(spec, got, want)
    single = set(name for name, shp in spec.layout() if int(np.prod(shp)) == 1)
    scale = float(np.linalg.norm(np.asarray(want, np.float64))) / np.sqrt(len(want)) + 1e-30
    tol = lambda name: max(rel, (rel_of or {}).get(name, 0.0))
    bad = [r for r in rows if r[2] > tol(r[0]) and r[1] > tol(r[0]) * scale and not (r[0] in single and r[1] <= abs_floor)]
    msg = "\n".join("%-28s max_abs=%.3e rel_l2=%.3e" % r for r in rows)
    assert not bad, "%s mismatch (rel tol %g):\n%s" % (what, rel, msg)


def device_pool_codes(net, B):
    """arg-max codes (0..3) of the 2x2 pooling windows of the device network's last forward, per conv layer."""
    from cartpoleplusplus_amd._lib import lib, check, ptr
    out = {}
    for i, (name, _k, _co) in enumerate(O.CONV_DEFS):
        shp = getattr(net, "pool%d" % (i + 1)).get_shape()
        codes = np.empty((B,) + tuple(shp[1:]), np.float32)
        check(lib.cpp_net_get_pool(net.handle, 11 + i, B, ptr(codes)))
        out[name] = codes.astype(np.uint8)
    return out


def assert_grads_close_modulo_pool_ties(spec, device_net, B, oracle_net, oracle_cache_fn, oracle_grads_fn, got,
                                        what="", rel=2e-5, margin_tol=1e-5):
    """Gradient parity with the max-pool's discontinuity taken into account.  The pool routes a window's gradient
    to its arg-max; where the two largest pre-activations of a window agree to rounding level, a different (but
    equally valid) f32 summation order picks the other element and moves that gradient to a neighbouring pixel.
    Such a flip is accepted only if the oracle itself sees a near tie there (margin <= margin_tol relative); the
    oracle's gradient is then recomputed with the device's choice at exactly those windows and must match."""
    want = oracle_grads_fn()
    try:
        assert_flat_close(spec, got, want, rel=rel, what=what)
        return 0
    except AssertionError as e:
        first = e
    cache = oracle_cache_fn()
    codes = device_pool_codes(device_net, B)
    flips = 0
    for name, _k, _co in O.CONV_DEFS:
        _x, pooled, amax, _h, _w = cache[name]
        margin = cache[name + ":margin"]
        diff = (codes[name] != amax) & (pooled > 0)
        bad = diff & (margin > margin_tol * np.maximum(1.0, np.abs(pooled)))
        assert not bad.any(), "%s: %s arg-max differs at %d window(s) that are not near ties\n%s" % (
            what, name, int(bad.sum()), first)
        flips += int(diff.sum())
    assert flips > 0, first
    oracle_net.amax_override = codes
    try:
        want = oracle_grads_fn()
    finally:
        oracle_net.amax_override = None
    assert_flat_close(spec, got, want, rel=rel,
                      what="%s (oracle re-run with the device's choice at %d near-tie pooling windows)" % (what, flips))
    return flips


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al.), the generator of the replay sampler and of the dropout masks."""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & 0xFFFFFFFF, p1 & 0xFFFFFFFF,
             ((p0 >> 32) ^ c[3] ^ k[1]) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
        k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
    return c


def dropout_masks(namespace, hidden, B, step):
    """the keep masks the device draws for the `step`-th training-mode forward of network `namespace`
    (include/cartpolepp_abi.h, cpp_net_spec.use_dropout): {'h<i>': (B, units) of 0/1}.  Word 0 of
    philox4x32_10([row * units + unit, layer, step & 0xFFFFFFFF, step >> 32], [crc32(namespace), 0]), lowest bit -- computed with
    the vectorised philox4x32_10_np (tests/test_dropout_sensitivity.py holds the two to each other bit for bit)."""
    import zlib
    seed = zlib.crc32(namespace.encode()) & 0xffffffff
    step = int(step)
    out = {}
    for layer, units in enumerate(hidden):
        idx = np.arange(B * units, dtype=np.uint64)
        assert B * units <= 1 << 32
        w0 = philox4x32_10_np(idx, np.full_like(idx, layer), np.full_like(idx, step & 0xFFFFFFFF), np.full_like(idx, step >> 32), seed, 0)[0]
        out["h%d" % layer] = (w0 & np.uint64(1)).astype(np.float64).reshape(B, units)
    return out


def set_actor_masks(ref, B, count):
    """hand an oracle DDPG (or a restatement built on it) the masks of training-mode forward number `count` of the actor and of the
    target actor; nothing to do without --use-dropout"""
    spec = ref.actor.spec
    if spec.dropout:
        ref.actor.drop_masks = dropout_masks("actor", spec.hidden, B, count)
        ref.target_actor.drop_masks = dropout_masks("target_actor", spec.hidden, B, count)


def device_relu_active(net, B):
    """which pooled conv outputs of the device network's last forward are > 0 (the cells its backward lets gradient through)."""
    return {name: getattr(net, "pool%d" % (i + 1)).eval(B) > 0 for i, (name, _k, _co) in enumerate(O.CONV_DEFS)}


def relu_flips_are_at_the_boundary(cache, device_active, tol=1e-5, what=""):
    """a forward cache of the oracle vs the device's ReLU decisions on the pooled conv outputs: where they differ, the oracle's
    own pre-activation maximum must be zero to rounding (|z| <= tol) -- max(z, 0) is continuous there but its gradient is not.
    Returns the number of such cells."""
    flips = 0
    for name, _k, _co in O.CONV_DEFS:
        _x, pooled, _amax, _h, _w = cache[name]
        zmax = cache[name + ":zmax"]
        diff = np.asarray(device_active[name]).reshape(pooled.shape) != (pooled > 0)
        bad = diff & (np.abs(zmax) > tol)
        assert not bad.any(), "%s: %s ReLU decision differs at %d cell(s) that are not at the boundary (largest |z| %.3e)" % (
            what, name, int(bad.sum()), float(np.abs(zmax[bad]).max()))
        flips += int(diff.sum())
    return flips


def pool_flips_are_near_ties(cache, device_codes, margin_tol=1e-5, what=""):
    """a forward cache computed with `amax_override = device_codes`: wherever the device routed a pooling window to another
    element than the oracle's own arg-max (and the pooled value is positive, i.e. the route carries gradient), the oracle
    must itself see a near tie there -- two largest pre-activations within margin_tol (relative to max(1, |value|)).
    Returns the number of such windows."""
    flips = 0
    for name, _k, _co in O.CONV_DEFS:
        _x, pooled, _amax, _h, _w = cache[name]
        own, margin = cache[name + ":amax_own"], cache[name + ":margin"]
        diff = (np.asarray(device_codes[name]).reshape(own.shape) != own) & (pooled > 0)
        bad = diff & (margin > margin_tol * np.maximum(1.0, np.abs(pooled)))
        assert not bad.any(), "%s: %s arg-max differs at %d window(s) that are not near ties (largest margin %.3e)" % (
            what, name, int(bad.sum()), float(margin[bad].max()))
        flips += int(diff.sum())
    return flips


def fill_with_rendered_episodes(agent, shape, rows, seed=0, blind_camera=False, as_u8=False, glint=0.0, opts=None):
    """`rows` transitions of random-policy episodes of the software-rasterised cart and pole (synthetic_env.RasterCartpole: flat
    backgrounds, R nearly identical repeat frames, optionally a camera that sees one colour only) into the agent's replay memory,
    through ReplayMemory.add_episode as the reference's rollout loop does (ddpg_cartpole.py:315-326)."""
    from cartpoleplusplus_amd import ddpg_cartpole as D
    from cartpoleplusplus_amd.synthetic_env import RasterCartpole, play_episodes
    env = RasterCartpole(opts if opts is not None else D.opts, seed=seed + 1, blind_camera=blind_camera, glint=glint)
    for first, seq in play_episodes(env, rows, np.random.default_rng(seed + 2)):
        if as_u8:
            first = np.rint(first * 255).astype(np.uint8)
            seq = [(a, r, np.rint(s2 * 255).astype(np.uint8)) for a, r, s2 in seq]
        agent.replay_memory.add_episode(first, seq)
    assert agent.replay_memory.size() == rows


F32_GRAD_FACTOR = 1.5


# ---- which kernels ran the heads: one eager, profiled minibatch, its launch counts against the ones the layer lists imply
def ddpg_gemm_levels(path, actor_hidden, critic_hidden, pixel):
    """GEMM launches of one DDPG minibatch (rt_ddpg_pass.cpp compute_gradients: the op graph launches every GEMM that is ready at
    once, so this is the number of levels that hold one).  na = actor layers with the head.  Fused heads (pixel critic: two
    levels in front of its action splice): the forward of the actors' first na - 1 - pre layers and the critics' prefix side by
    side, the heads kernel, then their backward chains side by side -- pre, the actor's last hidden layer in the heads kernel,
    takes one level off each actor chain.  GEMM levels: the actors, the critics' prefix, the concat layer and q three times over
    (fed actions, a = mu(s1), the target), dQ/da back to the splice, the actor's head gradient, the two backward chains."""
    na = len(actor_hidden) + 1
    if path in ("heads", "heads+pre"):
        assert pixel, "the fused heads need the pixel critic's prefix"
        return 2 * max(na - 1 - (path == "heads+pre"), 2)
    if pixel:
        return max(2 * na + 4, na + 7)
    return 2 * na + 2 * (len(critic_hidden) + 1)


def naf_gemm_levels(path, hidden, share):
    """the same for one NAF minibatch (rt_naf.cpp naf_compute_gradients, pixel trunk).  nh hidden layers.  heads: the nh layers
    forward, naf_heads_kernel (the head layers, d(representation)), nh levels of dW / dX; mlp (nh = 2): the second layer joins the
    kernel both ways; gemm: the three head layers and the target value's last layer take a level, naf_head_kernel, the heads' dW
    and the three accumulating d(representation) GEMMs, then the hidden stack; own trunks: three stacks side by side."""
    nh = len(hidden)
    if not share:
        assert path == "gemm"
        return 2 * nh + 2
    return {"mlp": 2, "heads": 2 * nh, "gemm": 2 * nh + 4}[path]


def _profiled_calls(ctx, fn):
    """launch counts per kernel family of fn() (profiling: the eager launch sequence, no graph capture)"""
    ctx.sync()
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        fn()
        ctx.sync()
    finally:
        ctx.prof_enable(False)
    prof = ctx.prof_read()
    ctx.prof_reset()
    return {k: n for k, (_ms, n) in prof.items()}


def _profiled_step(agent, ctx, B):
    return _profiled_calls(ctx, lambda: agent.train_step(B, 1))


def ddpg_path(agent, B, actor_hidden, critic_hidden, pixel):
    """one eager minibatch on the replay memory's rows, profiled: 'heads+pre', 'heads' or 'gemm' ('heads+pre|heads' where the
    two launch the same number of GEMM levels: an actor of two hidden layers, whose folded layer is hidden behind the critics'
    two-level prefix).  Raises if the counts fit none of them."""
    n = _profiled_step(agent, agent.actor.ctx, B)
    heads, gemm = n.get("heads", 0), n.get("gemm", 0)
    cand = ["heads+pre", "heads"] if heads == 1 else ["gemm"] if heads == 0 else []
    if "heads+pre" in cand and len(actor_hidden) < 2:
        cand.remove("heads+pre")
    fit = [p for p in cand if ddpg_gemm_levels(p, actor_hidden, critic_hidden, pixel) == gemm]
    assert fit, "launch counts %s fit no DDPG head path (actor %s, critic %s)" % (n, actor_hidden, critic_hidden)
    return "|".join(fit)


def naf_path(agent, B, hidden, share, dropout=False):
    """the same for NAF: 'mlp' (naf_mlp_kernel), 'heads' (naf_heads_kernel) or 'gemm' (GEMM levels + naf_head_kernel).
    dropout: naf_mlp_kernel knows no masks and is no candidate (launch counts that fit only 'mlp' then fit nothing)."""
    n = _profiled_step(agent, agent.value_net.ctx, B)
    gemm = n.get("gemm", 0)
    assert n.get("naf_head", 0) == 1, n
    cand = (["mlp"] if len(hidden) == 2 and not dropout else []) + ["heads", "gemm"] if share else ["gemm"]
    fit = [p for p in cand if naf_gemm_levels(p, hidden, share) == gemm]
    assert len(fit) == 1, "launch counts %s fit %s of the NAF head paths (hidden %s, share %s)" % (n, fit, hidden, share)
    return fit[0]


# ---- which kernels ran the conv trunk: the profiler families that are alternatives of each other (rt_core.cpp's names; conv.hip books
# ---- conv1 under *_f16 when conv_k16.h / conv_rs16.h / conv_dw16.h took the launch, the pair launches under conv<i>_bwd)
CONV_ROUTE_FAMILIES = (("conv1_fwd", ("conv1_fwd_f16", "conv1_fwd")),
                       ("conv1_dw", ("conv1_dw_f16", "conv1_dw_gather", "conv1_dw")),
                       ("conv2_bwd", ("conv2_bwd", "conv2_dx", "conv2_dw")),
                       ("conv3_bwd", ("conv3_bwd", "conv3_dx", "conv3_dw")),
                       ("stats", ("stats_generic", "gather_stats", "reduce_gather")))


def conv_routes_of(calls):
    """launch counts per family -> {part of the trunk: the families that launched for it, joined with '+' in CONV_ROUTE_FAMILIES' order}
    and 'conv3_fwd': whether conv3's forward had a launch of its own (False: the tail of conv2's, conv23_fuse_ok)."""
    out = {part: "+".join(f for f in fams if calls.get(f, 0) > 0) for part, fams in CONV_ROUTE_FAMILIES}
    out["conv3_fwd"] = calls.get("conv3_fwd", 0) > 0
    return out


def conv_routes(agent, B):
    """one eager minibatch on the replay memory's rows, profiled: which kernel families ran conv1's forward ('conv1_fwd_f16': the f16
    pipes, 'conv1_fwd': the f32-input kernels), conv1's dW ('conv1_dw_f16' / 'conv1_dw_gather', or 'conv1_dw'), conv2's and conv3's
    backward ('conv<i>_bwd': one launch, or 'conv<i>_dx+conv<i>_dw'), the sample pass's statistics, and whether conv3's forward launched
    on its own.  A part that nothing launched for is ''; conv1 on two routes at once would read 'conv1_fwd_f16+conv1_fwd'."""
    return conv_routes_of(_profiled_step(agent, agent.actor.ctx, B))


def fused_step_against_f64_oracle(shape, B, rows, replay_store="f16", replay_size=None, seed=0, graph=True,
                                  atol=1e-5, grad_rel=2e-5, param_rel=2e-6, warm="philox", report_only=False,
                                  fill="noise", f32_twin=False, flip_tol=1e-5, probe=False, before_step=None, pixel=True, hyper=None,
                                  prepare=None, host_seed=None, probe_conv=False, capacity=None, **pair_kw):
    """ONE minibatch of the fused inner step (cpp_ddpg_train_step, default kernels: f16-pipe conv1 reading the replay store
    through the sampled slots, bf16-pipe conv2, fused heads, paired launches) -- with graph=True the hipGraph REPLAY of it,
    on rows drawn by the device's Philox sampler -- against oracle.DDPG(float64) on the same rows and the same starting
    parameters: actions / Q / TD / dQ/da at `atol` (north_star: 1e-5), both pre-clip gradient lists per variable at
    `grad_rel` (pool routes: the device's, accepted only at near ties), the clipped SGD result and the target updates.
    pair_kw: make_pair's widths, action size and options (--use-dropout: the oracle draws the device's masks).  probe: one
    profiled minibatch first, report["path"] = ddpg_path().  probe_conv: the same, report["conv"] = conv_routes().  before_step(): called right before the minibatch that is checked.
    pixel=False: a low-dimensional state of `shape` (no trunk: the pool and ReLU routes are not compared).  hyper: an O.Hyper the
    device agent and the oracle are both built with (None: the reference's defaults).  prepare(agent): called on the fresh agent, before
    anything runs (edge-case parameters).  host_seed: parameters, episodes and (graph=False) rows are host_case(shape, B, 1, host_seed,
    rows)'s, so that a CPU-only test can compute from the same numbers (tests/test_batchnorm_sensitivity.py).  use_batch_norm=True
    (pair_kw): the pool codes and ReLU decisions read back are bn_relu_pool_kernel's, the oracle normalises with the batch moments in
    all four networks.  report["grads"]: the device's two pre-clip lists.
    capacity=C > B: the agent is built for batches of C rows and the checked minibatch of B rows comes behind a C-row one (eager, and
    with graph=True its capture and a replay) that leaves real data in every workspace row, partial slot and noise buffer, and behind
    one B-row step (eager, with graph=True the capture); one more C-row step follows and is held to the oracle at the same bars
    (report["back"]: its report).  probe / probe_conv then profile the B-row minibatch on the capacity-C agent."""
    import ctypes
    from cartpoleplusplus_amd import _lib
    if hyper is not None:
        pair_kw.update(hyper_options(hyper))
    case = None
    if host_seed is not None:
        case = host_case(shape, B, 1, host_seed, rows=rows, batch_norm=bool(pair_kw.get("use_batch_norm", False)))
        pair_kw = dict(pair_kw, perturb=False)
    agent, _ref, (aspec, cspec) = make_pair(shape, B, pixel, seed=seed, replay_size=replay_size or rows + 50,
                                           replay_store=replay_store, capacity=capacity, **pair_kw)
    report = {}
    steps = 0                                             # training-mode forwards before the one checked (dropout masks)
    try:
        rm = agent.replay_memory
        if case is not None:
            for net, p in zip(agent.networks(), case[1]):
                assert net.get_params().shape == p.shape
                net.set_params(p)
        if prepare is not None:
            prepare(agent)
        if case is not None:
            for ep in case[2]:
                rm.add_episode(*ep)
            assert rm.size() == rows
        elif fill == "noise":
            rm.fill_synthetic(rows, seed=21 + seed)
        else:
            assert fill in ("render", "render-blind", "render-glint"), fill
            fill_with_rendered_episodes(agent, shape, rows, seed=seed, blind_camera=(fill != "render"),
                                        glint=0.02 if fill == "render-glint" else 0.0)
        C = B if capacity is None else int(capacity)
        assert C >= B
        rows_of = lambda n, salt: np.random.default_rng(seed + salt).integers(0, rows, n).astype(np.int32)
        if C > B:                                         # a full-capacity minibatch first: every row and slot holds real data
            if graph:
                agent.train_step(C, 1)                    # eager pass + capture
                agent.train_step(C, 1)                    # replay
                steps += 2
            else:
                agent.train_step(C, 1, idxs=rows_of(C, 6))
                steps += 1
        if probe:
            report["path"] = ddpg_path(agent, B, aspec.hidden, cspec.hidden, pixel)
            steps += 1
        if probe_conv:
            report["conv"] = conv_routes(agent, B)
            steps += 1
        if graph or warm == "philox-eager":
            agent.train_step(B, 1)                        # eager pass + capture
            steps += 1
        elif warm == "rows" or C > B:
            agent.train_step(B, 1, idxs=rows_of(B, 77))
            steps += 1
        nets = (agent.actor, agent.critic, agent.target_actor, agent.target_critic)

        def step_and_read(Bx, idxs, before=None):
            """one minibatch of Bx rows (idxs None: the device's draw, a replay where this key's graph is held) and what it left"""
            d = {"B": Bx, "steps": steps, "P": [n.get_params() for n in nets]}
            if before is not None:
                before()
            if idxs is None:
                agent.train_step(Bx, 1)
                idxs = np.empty(Bx, np.int32)
                _lib.check(_lib.lib.cpp_replay_last_indexes(rm.handle, Bx, idxs.ctypes.data_as(ctypes.c_void_p)))
            else:
                agent.train_step(Bx, 1, idxs=idxs)        # same launch sequence, eager, caller's rows
            assert idxs.min() >= 0 and idxs.max() < rows and len(np.unique(idxs)) > Bx // 2
            d["values"] = agent.trainer.last_values(Bx)
            d["grads"] = (agent.actor.get_grads(), agent.critic.get_grads())
            d["stats"] = agent.trainer.last_stats()
            d["Pn"] = [n.get_params() for n in nets]
            if pixel:
                d["codes"] = (device_pool_codes(agent.actor, Bx), device_pool_codes(agent.critic, Bx))
                d["relu"] = (device_relu_active(agent.actor, Bx), device_relu_active(agent.critic, Bx))
                d["pools_c"] = [getattr(agent.critic, "pool%d" % i).eval(Bx) for i in (1, 2, 3)]
            else:
                d["codes"] = d["relu"] = (None, None)
            # the minibatch, read back through paths that do not involve the gather kernel's state copy
            s1, s2 = rm.state[rm.state_1_idx[idxs]], rm.state[rm.state_2_idx[idxs]]
            hb = rm.batch(idxs=idxs)
            a, r, m = hb.action, hb.reward, hb.terminal_mask
            assert np.array_equal(m[:, 0], rm.terminal_mask[idxs, 0]) and np.array_equal(r[:, 0], rm.reward[idxs, 0])
            d["batch"] = (s1, a, r, m, s2)
            return d

        checked = step_and_read(B, None if graph else rows_of(B, 5) if case is None else case[3], before_step)
        steps += 1
        back = step_and_read(C, None if graph else rows_of(C, 8)) if C > B else None      # the way back: no count of the small batch survives
    finally:
        agent.close()
    check_kw = dict(pixel=pixel, hyper=hyper, atol=atol, grad_rel=grad_rel, param_rel=param_rel, report_only=report_only,
                    f32_twin=f32_twin, flip_tol=flip_tol)
    report = _check_fused_step(checked, aspec, cspec, report, **check_kw)
    if back is not None:
        report["back"] = _check_fused_step(back, aspec, cspec, {}, **check_kw)
    return report


def _check_fused_step(d, aspec, cspec, report, pixel, hyper, atol, grad_rel, param_rel, report_only, f32_twin, flip_tol):
    """what fused_step_against_f64_oracle's step_and_read() brought back from one minibatch against oracle.DDPG(float64) started from
    the parameters read just before it"""
    B, steps, P, Pn, stats = d["B"], d["steps"], d["P"], d["Pn"], d["stats"]
    actions, dq_da, q, td = d["values"]
    g_a, g_c = d["grads"]
    (codes_a, codes_c), (relu_a, relu_c), pools_c = d["codes"], d["relu"], d.get("pools_c")
    s1, a, r, m, s2 = d["batch"]
    report["grads"] = (g_a, g_c)
    report["norms"] = (float(stats[1]), float(stats[2]))  # (pre-clip, actor's and critic's lists: which side of a clip they fall on)
    ref = O.DDPG(aspec, cspec, P[0], P[1], np.float64, **({} if hyper is None else {"hyper": hyper}))
    ref.set_targets(P[2], P[3])
    if aspec.dropout:
        ref.actor.drop_masks = dropout_masks("actor", aspec.hidden, B, steps)
        ref.target_actor.drop_masks = dropout_masks("target_actor", aspec.hidden, B, steps)
    # the two discontinuities of the trunk's gradient -- which element of a 2x2 window carries it, and whether the ReLU lets it
    # through -- are taken from the device and must coincide with the oracle's own except at rounding-level ties
    ref.actor.amax_override, ref.critic.amax_override = codes_a, codes_c
    ref.actor.relu_override, ref.critic.relu_override = relu_a, relu_c
    t = (s1, a, r, m, s2)
    ag = ref.actor_gradients(s1)
    cg = ref.critic_gradients(t)
    for key, fn, args in (("flips_actor", pool_flips_are_near_ties, (ag["cache_actor"], codes_a)),
                          ("flips_critic", pool_flips_are_near_ties, (cg["cache_critic"], codes_c)),
                          ("relu_flips_actor", relu_flips_are_at_the_boundary, (ag["cache_actor"], relu_a)),
                          ("relu_flips_critic", relu_flips_are_at_the_boundary, (cg["cache_critic"], relu_c))) if pixel else ():
        try:
            report[key] = fn(*args, flip_tol, what=key.split("_")[-1])
        except AssertionError as e:
            if not report_only:
                raise
            report[key] = "FAILED: %s" % e
    report["err_actions"] = float(np.abs(actions - ag["actions"]).max())
    report["err_dq_da"] = float(np.abs(dq_da - ag["dq_da"]).max())
    report["err_q"] = float(np.abs(q - cg["q"]).max())
    report["err_td"] = float(np.abs(td - cg["td"]).max())
    report["q_scale"] = float(np.abs(cg["q"]).max())
    for i, (name, _k, _co) in enumerate(O.CONV_DEFS if pixel else ()):
        want = cg["cache_critic"][name][1]
        report["err_pool%d" % (i + 1)] = float(np.abs(pools_c[i].reshape(want.shape) - want).max())
        report["mag_pool%d" % (i + 1)] = float(np.abs(want).max())
    if f32_twin:
        # the same evaluation in float32 numpy (the rounding an f32 implementation such as the reference's TF CPU kernels is
        # entitled to): how far IT sits from the float64 values on these inputs
        ref32 = O.DDPG(aspec, cspec, P[0], P[1], np.float32, **({} if hyper is None else {"hyper": hyper}))
        ref32.set_targets(P[2], P[3])
        if aspec.dropout:
            ref32.actor.drop_masks, ref32.target_actor.drop_masks = ref.actor.drop_masks, ref.target_actor.drop_masks
        ref32.actor.amax_override, ref32.critic.amax_override = codes_a, codes_c      # (the same routes: rounding is what is compared)
        ref32.actor.relu_override, ref32.critic.relu_override = relu_a, relu_c
        ag32, cg32 = ref32.actor_gradients(s1), ref32.critic_gradients(t)
        f32_rel_a = {n: F32_GRAD_FACTOR * r_ for n, _m, r_ in per_var_report(aspec, ag32["grads"], ag["grads"])}
        f32_rel_c = {n: F32_GRAD_FACTOR * r_ for n, _m, r_ in per_var_report(cspec, cg32["grads"], cg["grads"])}
        report["f32_rel_actor_grads"] = max(f32_rel_a.values()) / F32_GRAD_FACTOR
        report["f32_rel_critic_grads"] = max(f32_rel_c.values()) / F32_GRAD_FACTOR
        report["f32_err_actions"] = float(np.abs(ag32["actions"] - ag["actions"]).max())
        report["f32_err_dq_da"] = float(np.abs(ag32["dq_da"] - ag["dq_da"]).max())
        report["f32_err_q"] = float(np.abs(cg32["q"] - cg["q"]).max())
        report["f32_err_td"] = float(np.abs(cg32["td"] - cg["td"]).max())
        for i, (name, _k, _co) in enumerate(O.CONV_DEFS if pixel else ()):
            report["f32_err_pool%d" % (i + 1)] = float(np.abs(cg32["cache_critic"][name][1] - cg["cache_critic"][name][1]).max())
        report["white_scale_max"] = float(np.max(cg["cache_critic"]["white"][0]))
        report["white_scale_min"] = float(np.min(cg["cache_critic"]["white"][0]))
    if report_only:
        report["events"] = {k: report[k] for k in report if "flips" in k}
        report["actor"] = [(n, "%.2e" % r_) for n, _m, r_ in per_var_report(aspec, g_a, ag["grads"])][:6]
        report["critic"] = [(n, "%.2e" % r_) for n, _m, r_ in per_var_report(cspec, g_c, cg["grads"])][:6]
        return report
    assert report["err_actions"] < atol and report["err_dq_da"] < atol, report
    assert report["err_q"] < atol and report["err_td"] < atol, report
    assert abs(stats[0] - cg["loss"]) < atol * max(1.0, abs(cg["loss"])), (stats, cg["loss"])
    # (f32_twin: a variable's gradient may be as far from float64 as F32_GRAD_FACTOR x the float32 numpy evaluation's -- the critic's
    # gradients are linear in TD, and on correlated minibatches (renders) sum_b td_b cancels: 5e-6 on TD is 5e-5 of the head's gradient)
    assert_flat_close(aspec, g_a, ag["grads"], rel=grad_rel, what="actor pre-clip grads vs f64 oracle", rel_of=f32_rel_a if f32_twin else None)
    try:
        assert_flat_close(cspec, g_c, cg["grads"], rel=grad_rel, what="critic pre-clip grads vs f64 oracle",
                          abs_floor=2.0 * report["err_td"], rel_of=f32_rel_c if f32_twin else None)
    except AssertionError:
        # the critic's gradients are LINEAR in TD: g = (2 / B) sum_b td_b dq_b/dtheta.  On a correlated minibatch (consecutive
        # renders) the td_b nearly cancel in that sum and the TD error admitted above (< atol) is a large fraction of what is left.
        # Second chance: the oracle's backward pass fed with the DEVICE's TD values -- the backward arithmetic alone, at grad_rel
        cg_dev = ref.critic_gradients(t, td_override=td)
        assert_flat_close(cspec, g_c, cg_dev["grads"], rel=grad_rel, what="critic pre-clip grads vs f64 oracle's backward pass of the device's TD")
        report["critic_grads_checked_at_device_td"] = True
        nc_dev = float(np.linalg.norm(cg_dev["grads"]))
    report["rel_actor_grads"] = max(r_[2] for r_ in per_var_report(aspec, g_a, ag["grads"]))
    report["rel_critic_grads"] = max(r_[2] for r_ in per_var_report(cspec, g_c, cg["grads"]))
    na, nc = float(np.linalg.norm(ag["grads"])), float(np.linalg.norm(cg["grads"]))
    # (the reported critic norm is the norm of the gradient checked above: where that check needed the device's TD values -- B = 1 with a
    # TD of 1e-2: the admitted 1e-5 on TD is 1e-3 of the gradient -- the norm is held to the same gradient; rs16_geometry_parity.py 601, draw 1)
    nc_ref = nc_dev if report.get("critic_grads_checked_at_device_td") else nc
    assert abs(stats[1] - na) < 1e-4 * max(1.0, na) and abs(stats[2] - nc_ref) < 1e-4 * max(1.0, nc_ref), (stats, na, nc, nc_ref)
    # clip + SGD (util.py:47-50, ddpg_cartpole.py:118-119,218) and the target updates (:336-337) on top of them
    hp = O.DEFAULT_HYPER if hyper is None else hyper
    ca, _ = O.clip_by_global_norm(ag["grads"], hp.gradient_clip, np.float64)
    cc, _ = O.clip_by_global_norm(cg["grads"], hp.gradient_clip, np.float64)
    want_a, want_c = P[0] - hp.actor_lr * ca, P[1] - hp.critic_lr * cc
    assert_flat_close(aspec, Pn[0], want_a, rel=param_rel, what="actor params after the step")
    assert_flat_close(cspec, Pn[1], want_c, rel=param_rel, what="critic params after the step")
    assert_flat_close(aspec, Pn[2], O.soft_update(P[2], want_a, hp.target_update_rate, np.float64), rel=1e-6, what="target actor")
    assert_flat_close(cspec, Pn[3], O.soft_update(P[3], want_c, hp.target_update_rate, np.float64), rel=1e-6, what="target critic")
    # the update itself (not hidden behind the much larger parameters): delta vs -lr * clipped gradient
    for name, new, old, want in (("actor", Pn[0], P[0], want_a), ("critic", Pn[1], P[1], want_c)):
        d_got, d_want = new.astype(np.float64) - old, want - old
        report["rel_delta_" + name] = float(np.linalg.norm(d_got - d_want) / np.linalg.norm(d_want))
        # f32 parameters: storing theta - lr*g rounds at |theta| * 2^-24 per element, on top of the gradient's own error
        # (... which, with f32_twin, may be as far from float64 as F32_GRAD_FACTOR x the float32 numpy evaluation's own gradients are: on
        # nearly constant channels that is 1e-3, not 5e-5)
        rel_d = max(5e-5, F32_GRAD_FACTOR * report["f32_rel_%s_grads" % name]) if f32_twin else 5e-5
        bound = 2.0 ** -23 * np.linalg.norm(old) + rel_d * np.linalg.norm(d_want)
        assert np.linalg.norm(d_got - d_want) < bound, (name, report, bound)
    # ... and the soft update's own delta, -tau * (target - new source): the rel=1e-6 asserts above are relative to the target,
    # 1 / tau times larger than what the update adds to it.  Same form: f32 storage rounding of the target plus the relative bar
    for name, new, old, src in (("target_actor", Pn[2], P[2], want_a), ("target_critic", Pn[3], P[3], want_c)):
        d_got = new.astype(np.float64) - old
        d_want = O.soft_update(old, src, hp.target_update_rate, np.float64) - old
        err, size = float(np.linalg.norm(d_got - d_want)), float(np.linalg.norm(d_want))
        report["rel_delta_" + name] = err / size if size > 0 else err
        bound = 2.0 ** -23 * np.linalg.norm(old) + 5e-5 * size
        assert err < bound, (name, report, bound)
    return report


def philox4x32_10_np(c0, c1, c2, c3, k0, k1):
    """vectorised Philox4x32-10: uint64 numpy arrays (values < 2^32) in, four uint32 words out."""
    M0, M1, W0, W1, MASK = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85, np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(x, np.uint64) for x in (c0, c1, c2, c3))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def synthetic_state_codes(slot, elems, seed):
    """the 8-bit pixel codes cpp_replay_fill_synthetic writes into state slot `slot` (csrc/replay.hip: byte e of the Philox block
    of flat position // 16, key = seed), regenerated on the host -- an independent witness for gathers from anywhere in a store
    of any size (64-bit positions)."""
    first = int(slot) * int(elems)
    blocks = np.arange(first // 16, (first + elems + 15) // 16, dtype=np.uint64)
    w = philox4x32_10_np(blocks & np.uint64(0xFFFFFFFF), blocks >> np.uint64(32), np.full_like(blocks, 0x5eed), np.full_like(blocks, 1),
                         seed & 0xFFFFFFFF, seed >> 32)
    by = np.stack([(w[e >> 2] >> np.uint64(8 * (e & 3))) & np.uint64(0xFF) for e in range(16)], axis=1).astype(np.uint8).ravel()
    off = first - int(blocks[0]) * 16
    return by[off:off + elems]


# ---- several minibatches at chosen hyperparameters: inputs made on the host, so that the oracle-only sensitivity test and the GPU
# ---- test compute from the same numbers (tests/test_hyper_sensitivity.py, tests/test_gpu_hyperparameters.py)
DEFAULT_ACTOR_HIDDEN = (100, 100, 50)          # --actor-hidden-layers' default (the pixel critic's stack is fixed: NetSpec._fc_layers)


def delta_bound(theta, d_want, r, nb=1):
    """how far a float32 update may sit from the float64 one: every one of `nb` stores of theta rounds at 2^-24 |theta| per element
    (2^-23 covers the fused multiply-add in front of it), and the update itself is held to `r` of its own size"""
    return 2.0 ** -23 * nb * float(np.linalg.norm(np.asarray(theta, np.float64))) + r * float(np.linalg.norm(d_want))


def host_case(shape, B, nb, seed, rows=24, action_dim=2, batch_norm=False, dropout=False, actor_hidden=None):
    """specs, starting parameters of the four DDPG networks (xavier + make_pair's perturbations), `rows` transitions as episodes
    (pixel: codes k / 255 in f16, what the replay store holds exactly) and nb * B row numbers with the minibatches they select.
    batch_norm: --use-batch-norm networks (the same numbers: the conv bias slots then hold BatchNorm/beta).  dropout: --use-dropout
    (the same numbers: the actor's spec asks for masks).  actor_hidden: --actor-hidden-layers (None: the default; other widths draw
    other numbers)."""
    from oracle.replay_np import OracleReplayMemory
    pixel = len(shape) == 5
    kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:])), batch_norm=batch_norm) if pixel else dict(pixel=False, state_elems=int(np.prod(shape)))
    aspec = O.NetSpec("actor", action_dim, DEFAULT_ACTOR_HIDDEN if actor_hidden is None else tuple(actor_hidden), dropout=dropout, **kw)
    cspec = O.NetSpec("critic", action_dim, DEFAULT_ACTOR_HIDDEN, **kw)
    rng = np.random.default_rng(1000 + seed)
    P = []
    for spec in (aspec, cspec):
        p = O.init_params(spec, rng)
        P.append(p + rng.normal(0, 0.05, p.shape).astype(np.float32))
    for p in list(P):
        P.append(p + rng.normal(0, 0.01, p.shape).astype(np.float32))
    orm = OracleReplayMemory(rows, shape, action_dim)
    mk = (lambda: rng.integers(0, 256, shape).astype(np.float16) / np.float16(255)) if pixel else \
         (lambda: rng.standard_normal(shape).astype(np.float32))
    episodes, left = [], rows
    while left > 0:
        n = min(left, int(rng.integers(2, 7)))
        episodes.append((mk(), [(rng.uniform(-1, 1, (1, action_dim)).astype(np.float32), float(rng.integers(0, 3)), mk()) for _ in range(n)]))
        orm.add_episode(*episodes[-1])
        left -= n
    idxs = rng.integers(0, rows, nb * B).astype(np.int32)
    batches = []
    for i in range(nb):
        ob = orm.batch(idxs=idxs[i * B:(i + 1) * B])
        batches.append((ob.state_1, ob.action, ob.reward, ob.terminal_mask, ob.state_2))
    return (aspec, cspec), P, episodes, idxs, batches


def oracle_of(specs, P, dt, hyper):
    ref = O.DDPG(specs[0], specs[1], P[0], P[1], dt, hyper=hyper)
    ref.set_targets(P[2], P[3])
    return ref


def four_vectors(ref):
    return [np.asarray(n.flat(), np.float64) for n in (ref.actor, ref.critic, ref.target_actor, ref.target_critic)]


def oracle_minibatch(ref, batch):
    """DDPG.train_minibatch, returning what the tests look at besides: both pre-clip norms and the trunk's routes -- per conv layer
    the 2x2 windows' arg-max where the window carries gradient (255 elsewhere), which is also the ReLU's decision"""
    dt, hp = ref.dt, ref.hp
    ag, cg = ref.actor_gradients(batch[0]), ref.critic_gradients(batch)
    routes = []
    for cache in (ag["cache_actor"], cg["cache_critic"]):
        for name, _k, _co in O.CONV_DEFS if ref.actor.spec.pixel else ():
            routes.append(np.where(cache[name][1] > 0, cache[name + ":amax_own"], 255).astype(np.uint8))
    a_clip, a_norm = O.clip_by_global_norm(ag["grads"], hp.gradient_clip, dt)
    c_clip, c_norm = O.clip_by_global_norm(cg["grads"], hp.gradient_clip, dt)
    ref.actor = O.Net(ref.actor.spec, (ref.actor.flat() - dt(hp.actor_lr) * a_clip).astype(dt), dt)
    ref.critic = O.Net(ref.critic.spec, (ref.critic.flat() - dt(hp.critic_lr) * c_clip).astype(dt), dt)
    return {"actor_norm": float(a_norm), "critic_norm": float(c_norm), "routes": routes, "td": cg["td"], "loss": float(cg["loss"])}


def oracle_train_step(ref, batches):
    outs = [oracle_minibatch(ref, b) for b in batches]
    ref.update_targets()
    return outs


def f32_twin_case(specs, P, batches, hyper):
    """the float64 oracle and its float32 numpy twin over the same minibatches + target update.  Returns (final f64 vectors, per vector
    r = max(5e-5, F32_GRAD_FACTOR x the twin's relative delta error), the f64 per-minibatch outputs, whether both took the same pool
    and ReLU routes in every minibatch)."""
    ref, ref32 = oracle_of(specs, P, np.float64, hyper), oracle_of(specs, P, np.float32, hyper)
    o64, o32 = oracle_train_step(ref, batches), oracle_train_step(ref32, batches)
    same = all(np.array_equal(x, y) for a, b in zip(o64, o32) for x, y in zip(a["routes"], b["routes"]))
    want, twin = four_vectors(ref), four_vectors(ref32)
    rs = []
    for w, t, p in zip(want, twin, P):
        d = np.linalg.norm(w - p)
        rs.append(max(5e-5, F32_GRAD_FACTOR * float(np.linalg.norm(t - w) / d) if d > 0 else 5e-5))
    return want, rs, o64, same


# the hyperparameter sets of tests/test_gpu_hyperparameters.py (each one's power is checked in tests/test_hyper_sensitivity.py)
LOUD = O.Hyper(1e-2, 5e-2, 0.9, 0.5, 0.25)                 # clip engaged on both lists
HYPER_SETS = {"LOUD": LOUD,
              "UNCLIPPED_NONE": LOUD._replace(gradient_clip=None),          # the kernel's clip <= 0
              "UNCLIPPED_1E4": LOUD._replace(gradient_clip=1e4),            # clip > 0 with a scale of exactly 1
              "SPLIT": LOUD._replace(gradient_clip=15.0)}                   # between the two lists' norms: one clipped, one not
ACTOR_LOUD = LOUD._replace(actor_lr=0.1)                   # an actor update as large as the critic's: a stale ACTOR image shows in the actor
RIDER_CASES = {"LOUD": ((64, 64, 3, 2, 3), 8, 1, LOUD), "ACTOR_LOUD": ((64, 64, 3, 2, 3), 8, 2, ACTOR_LOUD)}      # shape, B, host_case seed, set
SENS_SHAPE, SENS_B, SENS_SEED = (16, 16, 3, 1, 2), 16, 3
STALE_TARGET_CASE = ((64, 64, 3, 2, 3), 8, 2)              # shape, B, host_case seed
# batch-norm cases that tests/test_gpu_batchnorm_training.py runs on the device and tests/test_batchnorm_sensitivity.py plants faults in:
# shape, B, rows, host_case seed (batch_norm=True)
BN_B1_CASE = ((16, 16, 3, 1, 2), 1, 24, 41)               # a 2x2 conv3 output: four samples per channel
BN_B7_CASE = ((64, 64, 3, 1, 2), 7, 24, 42)               # bn_bwd_reduce_kernel's second pass
BN_PER_CASE = ((32, 32, 3, 2, 3), 8, 200, 1)              # the prioritized-replay case (the device draws its own rows: same shape, B, rows)
BN_HYPER_CASES = {"16x16x6": ((16, 16, 3, 1, 2), 8, 3), "64x64x18": ((64, 64, 3, 2, 3), 8, 1)}          # shape, B, host_case seed (64x64x18: the first seed
                                                                                                         # whose float32 twin keeps the float64 routes under all three sets); three minibatches
NAF_HYPER = dict(discount=0.9, target_update_rate=0.25, clip=0.5)
NAF_OPTIMISERS = {"momentum-0.5": ("Momentum", {"learning_rate": 0.01, "momentum": 0.5}, 1),       # name, args, warm-up steps
                  "momentum-0.0": ("Momentum", {"learning_rate": 0.01, "momentum": 0.0}, 1),
                  "adam-third-step": ("Adam", {"learning_rate": 0.01, "beta1": 0.8, "beta2": 0.9, "epsilon": 1e-3}, 2)}
NAF_RIDER_CASE = ((64, 64, 3, 2, 3), 8, 3, 30, 5)         # shape, B, minibatches, rows, seed: the shared trunk, conv1 on the operand image


def naf_host_case(shape, B, nb, rows, seed, hidden=(100, 50), action_dim=2, share=True, dropout=False, batch_norm=False):
    """host_case for the shared-trunk NAF agent: (value, mu, l) specs, the three parameter vectors + the target value network's,
    episodes, rows and the minibatches they select.  share=False: mu and l_values on trunks and hidden stacks of their own; dropout:
    --use-dropout; batch_norm: --use-batch-norm (the same numbers: the conv bias slots then hold BatchNorm/beta); a low-dimensional
    `shape` gives networks without a trunk."""
    from oracle import naf_np as N
    from oracle.replay_np import OracleReplayMemory
    if len(shape) == 5:
        kw = dict(pixel=True, H=shape[0], W=shape[1], C=int(np.prod(shape[2:])), dropout=dropout, batch_norm=batch_norm)
    else:
        kw = dict(pixel=False, state_elems=int(np.prod(shape)), dropout=dropout)
    if share:
        specs = (N.HeadSpec(1, "linear", list(hidden), **kw),
                 N.HeadSpec(action_dim, "tanh", [], False, state_elems=hidden[-1], head_only=True),
                 N.HeadSpec(N.num_l_values(action_dim), "linear", [], False, state_elems=hidden[-1], head_only=True))
    else:
        specs = (N.HeadSpec(1, "linear", list(hidden), **kw), N.HeadSpec(action_dim, "tanh", list(hidden), **kw),
                 N.HeadSpec(N.num_l_values(action_dim), "linear", list(hidden), **kw))
    rng = np.random.default_rng(2000 + seed)
    flats = []
    for sp in specs:
        p = N.init_head_params(sp, rng)
        flats.append(p + rng.normal(0, 0.05, p.shape).astype(np.float32))
    flats.append(flats[0] + rng.normal(0, 0.01, flats[0].shape).astype(np.float32))
    orm = OracleReplayMemory(rows, shape, action_dim)
    mk = (lambda: rng.integers(0, 256, shape).astype(np.float16) / np.float16(255)) if len(shape) == 5 else \
         (lambda: rng.standard_normal(shape).astype(np.float32))
    episodes, left = [], rows
    while left > 0:
        n = min(left, int(rng.integers(2, 6)))
        episodes.append((mk(), [(rng.uniform(-1, 1, (1, action_dim)).astype(np.float32), float(rng.integers(0, 3)), mk()) for _ in range(n)]))
        orm.add_episode(*episodes[-1])
        left -= n
    idxs = rng.integers(0, rows, nb * B).astype(np.int32)
    batches = []
    for i in range(nb):
        ob = orm.batch(idxs=idxs[i * B:(i + 1) * B])
        batches.append((ob.state_1, ob.action, ob.reward, ob.terminal_mask, ob.state_2))
    return specs, flats, episodes, idxs, batches


def naf_twin_case(specs, flats, batches, optimiser, optimiser_args, action_dim=2):
    """oracle.NAF.train_step (shared trunk, NAF_HYPER) in float64 and in float32 numpy.  Returns ((params, target) of the float64
    run, their r = max(5e-5, F32_GRAD_FACTOR x the twin's relative delta error), the float64 norms per minibatch, whether both took
    the same pool / ReLU routes in the value trunk in every minibatch)."""
    from oracle import naf_np as N
    refs, routes = {}, {}
    for dt in (np.float32, np.float64):
        r = N.NAF(specs[0], specs[1], specs[2], flats[0], flats[1], flats[2], True, action_dim, dt, discount=NAF_HYPER["discount"],
                  gradient_clip=NAF_HYPER["clip"], target_update_rate=NAF_HYPER["target_update_rate"],
                  optimiser=N.make_optimiser(optimiser, optimiser_args))
        r.target_value = O.Net(specs[0], flats[3], dt)
        routes[dt], norms = [], []
        for b in batches:
            cv = r._forward(b[0])[0]
            routes[dt] += [np.where(cv[c][1] > 0, cv[c + ":amax_own"], 255) for c, _k, _co in O.CONV_DEFS]
            norms.append(float(r.train(b)["norm"]))
        r.update_targets()
        refs[dt] = r
    same = all(np.array_equal(x, y) for x, y in zip(routes[np.float32], routes[np.float64]))
    want, rs = [], []
    for get, start in ((lambda r: r.flat(), np.concatenate(flats[:3])), (lambda r: r.target_value.flat(), flats[3])):
        w, t = np.asarray(get(refs[np.float64]), np.float64), np.asarray(get(refs[np.float32]), np.float64)
        want.append(w)
        rs.append(max(5e-5, F32_GRAD_FACTOR * float(np.linalg.norm(t - w) / np.linalg.norm(w - start))))
    return want, rs, norms, same


# ---- --use-dropout over several minibatches and several calls: the inputs and the float64 expectation that tests/test_gpu_dropout.py
# ---- holds the device to and tests/test_dropout_sensitivity.py plants faults in.  Minibatch k of call c is training-mode forward number
# ---- nb * c + k of every network with a dropout stack (include/cartpolepp_abi.h, cpp_net_spec.use_dropout)
DROP_PIX, DROP_LOWDIM = (16, 16, 3, 1, 2), (2, 2, 7)
DROP_B, DROP_NB, DROP_CALLS, DROP_ROWS, DROP_SEED = 6, 3, 2, 24, 7
DROP_NAF_OPTIMISER = ("Momentum", {"learning_rate": 0.01, "momentum": 0.5})
DROP_NAF_HIDDEN = {True: (100, 50), False: (32, 16)}          # share: the hidden stack (own trunks: test_gpu_head_shapes.py's widths)
NAF_DROP_NAMESPACES = ("value", "target_value", "naf/output_action", "naf/l_values")


def ddpg_dropout_case(shape):
    return host_case(shape, DROP_B, DROP_NB * DROP_CALLS, DROP_SEED, rows=DROP_ROWS, dropout=True)


def naf_dropout_case(shape, share):
    return naf_host_case(shape, DROP_B, DROP_NB * DROP_CALLS, DROP_ROWS, DROP_SEED, hidden=DROP_NAF_HIDDEN[share], share=share, dropout=True)


def ddpg_dropout_calls(specs, P, batches, dt=np.float64, hyper=LOUD, nb=DROP_NB, masks=dropout_masks, wrap=None):
    """oracle.DDPG over len(batches) / nb calls of nb minibatches + the target updates, the actor and the target actor drawing
    masks(namespace, hidden, B, nb * c + k) in minibatch k of call c.  wrap(ref): called before every minibatch (the sensitivity
    test swaps faulted networks in).  Returns per call (the four vectors after it, oracle_minibatch's outputs, a snapshot of the
    oracle after it)."""
    import copy
    ref = oracle_of(specs, P, dt, hyper)
    hidden, B = specs[0].hidden, int(np.asarray(batches[0][1]).shape[0])
    out = []
    for c in range(len(batches) // nb):
        outs = []
        for k in range(nb):
            count = nb * c + k
            if wrap is not None:
                wrap(ref)
            ref.actor.drop_masks = masks("actor", hidden, B, count)
            ref.target_actor.drop_masks = masks("target_actor", hidden, B, count)
            outs.append(oracle_minibatch(ref, batches[count]))
        ref.update_targets()
        out.append((four_vectors(ref), outs, copy.copy(ref)))
    return out


def naf_oracle(specs, flats, share, dt, optimiser=DROP_NAF_OPTIMISER, action_dim=2):
    from oracle import naf_np as N
    r = N.NAF(specs[0], specs[1], specs[2], flats[0], flats[1], flats[2], share, action_dim, dt, discount=NAF_HYPER["discount"],
              gradient_clip=NAF_HYPER["clip"], target_update_rate=NAF_HYPER["target_update_rate"], optimiser=N.make_optimiser(*optimiser))
    r.target_value = O.Net(specs[0], flats[3], dt)
    return r


def naf_dropout_calls(specs, flats, batches, share, dt=np.float64, nb=DROP_NB, masks=dropout_masks, wrap=None):
    """the same for oracle.NAF (NAF_HYPER, DROP_NAF_OPTIMISER): the masks are set before each train(), update_targets() once per call.
    Returns per call ((params, target value params), the pre-clip norms, the value trunk's routes per minibatch, a snapshot)."""
    import copy
    ref = naf_oracle(specs, flats, share, dt)
    hidden, B = specs[0].hidden, int(np.asarray(batches[0][1]).shape[0])
    out = []
    for c in range(len(batches) // nb):
        norms, routes = [], []
        for k in range(nb):
            count = nb * c + k
            if wrap is not None:
                wrap(ref)
            nets = (ref.value, ref.target_value) + (() if share else (ref.mu, ref.l))
            for net, ns in zip(nets, NAF_DROP_NAMESPACES):
                net.drop_masks = masks(ns, hidden, B, count)
            b = batches[count]
            cv = ref._forward(b[0])[0]
            routes += [np.where(cv[cn][1] > 0, cv[cn + ":amax_own"], 255) for cn, _k, _co in O.CONV_DEFS] if specs[0].pixel else []
            norms.append(float(ref.train(b)["norm"]))
        ref.update_targets()
        out.append(((np.asarray(ref.flat(), np.float64), np.asarray(ref.target_value.flat(), np.float64)), norms, routes, copy.copy(ref)))
    return out


def twin_rs(want, twin, start):
    """f32_twin_case's rule per vector: r = max(5e-5, F32_GRAD_FACTOR x the float32 numpy twin's relative delta error)"""
    rs = []
    for w, t, p in zip(want, twin, start):
        d = float(np.linalg.norm(w - p))
        rs.append(max(5e-5, F32_GRAD_FACTOR * float(np.linalg.norm(t - w)) / d) if d > 0 else 5e-5)
    return rs


# ---- batches below the capacity the agent was built with (tests/test_gpu_partial_batch.py, tests/test_partial_batch_host.py): four
# ---- minibatches of C, B, B and C rows on one agent of capacity C.  The C-row one leaves real data in every workspace row and partial
# ---- slot; the B-row ones must not see it; the last one must not see a count cached from the small ones.
PARTIAL_PIX, PARTIAL_LOWDIM = (16, 16, 3, 1, 2), (2, 2, 7)
PARTIAL_C, PARTIAL_B, PARTIAL_SEED = 8, 5, 11


def partial_sizes(C, B):
    return (C, B, B, C)


def _cut(idxs, batches, C, B):
    sizes = partial_sizes(C, B)
    return ([np.ascontiguousarray(idxs[i * C:i * C + n], dtype=np.int32) for i, n in enumerate(sizes)],
            [tuple(np.asarray(x)[:n] for x in batches[i]) for i, n in enumerate(sizes)])


def partial_case(shape, C=PARTIAL_C, B=PARTIAL_B, seed=PARTIAL_SEED, rows=24, **kw):
    """host_case drawn for four minibatches of C rows, the second and third cut to their first B rows: (specs, P, episodes, the four
    row lists, the four minibatches)"""
    specs, P, episodes, idxs, batches = host_case(shape, C, 4, seed, rows=rows, **kw)
    return (specs, P, episodes) + _cut(idxs, batches, C, B)


def naf_partial_case(shape, C=PARTIAL_C, B=PARTIAL_B, seed=PARTIAL_SEED, rows=24, **kw):
    """the same of naf_host_case"""
    specs, flats, episodes, idxs, batches = naf_host_case(shape, C, 4, rows, seed, **kw)
    return (specs, flats, episodes) + _cut(idxs, batches, C, B)


def minibatch_of_rows(rows, shape, action_dim, episodes, idxs):
    """the one-step minibatch rows `idxs` select from a memory of `rows` rows holding `episodes` (the oracle memory's own gather)"""
    from oracle.replay_np import OracleReplayMemory
    orm = OracleReplayMemory(rows, shape, action_dim)
    for ep in episodes:
        orm.add_episode(*ep)
    ob = orm.batch(idxs=np.asarray(idxs))
    return (ob.state_1, ob.action, ob.reward, ob.terminal_mask, ob.state_2)


def capacity_plan(rows, shape, action_dim, episodes, idxs, batches, B, capacity):
    """the minibatches of a variant case's run below the capacity: [(row list, minibatch)] of capacity, B, B and capacity rows -- the last
    `capacity` of the case's rows in front and behind, the case's first two minibatches between them"""
    assert capacity > B and len(idxs) >= max(capacity, 2 * B)
    big = np.ascontiguousarray(idxs[-capacity:], dtype=np.int32)
    wide = minibatch_of_rows(rows, shape, action_dim, episodes, big)
    return [(big, wide), (idxs[:B], batches[0]), (idxs[B:2 * B], batches[1]), (big, wide)]
