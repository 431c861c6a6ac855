"""The kernels between the hidden stacks and the first backward GEMMs at the widths, depths, action sizes and batch sizes users
can choose (--actor-hidden-layers, --critic-hidden-layers, --hidden-layers, the env's action size, --batch-size), not only at
the reference's defaults.  Each case first runs one profiled minibatch and asserts which path ran it -- DDPG: the heads kernel
with the actor's last hidden layer folded in ('heads+pre'), the heads kernel alone ('heads'), or GEMM levels + the TD kernel
('gemm'); NAF: naf_mlp_kernel ('mlp'), naf_heads_kernel ('heads'), or GEMM levels + naf_head_kernel ('gemm') -- and then holds one
minibatch of the fused step to the float64 oracle at the suite's bars (tests/helpers.py fused_step_against_f64_oracle,
tests/test_gpu_naf.py naf_fused_step_against_f64_oracle).  Small images: the trunk is cheap and the heads are what varies."""
import numpy as np
import pytest

from tests.helpers import fused_step_against_f64_oracle, make_pair

pytestmark = pytest.mark.gpu
PIX = (16, 16, 3, 1, 2)          # 16 x 16 render, one camera, two repeats: 6 channels
LOWDIM = (2, 2, 7)
DEFAULT_ACTOR = [100, 100, 50]


def _ddpg_case(actor_hidden, path, B=16, A=2, graph=False, **kw):
    rows = max(300, 2 * B)
    rep = fused_step_against_f64_oracle(PIX, B, rows, graph=graph, probe=True, actor_hidden=actor_hidden, action_dim=A, **kw)
    print("DDPG pixel actor %s A=%d B=%d: path %s (graph %s)" % (actor_hidden, A, B, rep["path"], graph))
    assert rep["path"] == path, (rep["path"], path)
    return rep


# (actor widths, expected path, graph replay).  The heads kernel (heads.hip, ddpg_heads_supported): n2a <= 64 (the actor's last
# width), n3 = n2c = 50 (the pixel critic's), A <= 8, B <= 1024; its folded layer (pre): >= 2 hidden layers, n1a <= 128, n2a even,
# (n1ap + 1) n2a + 68 <= 5120 floats.  At two hidden layers the folded layer saves no GEMM level -- the critics' two-level prefix
# is the longer chain -- and the launch counts cannot tell the two heads paths apart.
WIDTHS = [
    pytest.param(DEFAULT_ACTOR, "heads+pre", True, id="100-100-50-defaults"),
    pytest.param([100, 50], "heads+pre|heads", False, id="100-50"),
    pytest.param([64], "heads", True, id="64-one-layer"),
    pytest.param([100, 97, 50], "heads+pre", False, id="100-97-50-n1a-1-mod-4"),
    pytest.param([100, 65, 64], "heads+pre", False, id="100-65-64-n1a-1-mod-4-64-lanes"),
    pytest.param([100, 33, 50], "heads+pre", False, id="100-33-50-n1a-1-mod-4"),
    pytest.param([100, 98, 50], "heads+pre", False, id="100-98-50-n1a-2-mod-4"),
    pytest.param([100, 100, 63], "heads", False, id="100-100-63-odd-last-width"),
    pytest.param([100, 128, 38], "heads+pre", False, id="100-128-38-folded-input-limit"),
    pytest.param([100, 129, 30], "heads", False, id="100-129-30-one-past-it"),
    pytest.param([100, 128, 64], "heads", False, id="100-128-64-64-lanes"),
    pytest.param([100, 100, 65], "gemm", True, id="100-100-65-one-lane-past"),
    pytest.param([400, 300], "gemm", False, id="400-300-ddpg-paper"),
    pytest.param([4, 1, 2], "heads+pre", False, id="4-1-2-tiny"),
    pytest.param([16] * 8, "heads+pre", False, id="eight-layers-of-16"),
]


@pytest.mark.parametrize("actor_hidden,path,graph", WIDTHS)
def test_ddpg_pixel_actor_widths(actor_hidden, path, graph):
    _ddpg_case(actor_hidden, path, graph=graph)


# the heads kernel's instances: A = 1, 2, 4, 8 exact, 3 on the 4-wide one, 5..7 on the 8-wide one with padded lanes; A > 8: GEMMs
@pytest.mark.parametrize("A,path", [(1, "heads+pre"), (3, "heads+pre"), (4, "heads+pre"), (5, "heads+pre"), (8, "heads+pre"),
                                    (9, "gemm"), (16, "gemm")], ids=lambda v: str(v))
def test_ddpg_action_sizes(A, path):
    _ddpg_case(DEFAULT_ACTOR, path, A=A, graph=A == 5)


# one workgroup of the heads kernel runs 4 rows: B = 1 and 5 leave lanes without a row; 1024 is its last grid (256 workgroups)
@pytest.mark.parametrize("B,path", [(1, "heads+pre"), (5, "heads+pre"), (1024, "heads+pre"), (1025, "gemm")], ids=lambda v: str(v))
def test_ddpg_batch_edges(B, path):
    _ddpg_case(DEFAULT_ACTOR, path, B=B)


# low-dimensional critics take the action at layer 0 (no prefix in front of a splice): always the GEMM levels, K = state + A + 1
@pytest.mark.parametrize("actor_hidden,critic_hidden,graph", [([400, 300], [400, 300], False), ([17], [1], True), ([1], [17], False),
                                                              ([64] * 8, [64] * 8, False)],
                         ids=["400-300", "17-and-1", "1-and-17", "eight-layers-of-64"])
def test_ddpg_lowdim_widths(actor_hidden, critic_hidden, graph):
    rep = fused_step_against_f64_oracle(LOWDIM, 16, 300, graph=graph, probe=True, pixel=False, actor_hidden=actor_hidden,
                                        critic_hidden=critic_hidden, action_dim=3)
    print("DDPG low-dim actor %s critic %s: path %s" % (actor_hidden, critic_hidden, rep["path"]))
    assert rep["path"] == "gemm"


def test_ddpg_dropout_keeps_the_folded_layer_out():
    """--use-dropout at the widths that fold the layer without it: the heads kernel alone, with the x2 ReLU-gradient epilogue"""
    _ddpg_case([100, 97, 50], "heads", use_dropout=True)


def test_ddpg_prioritized_replay_on_a_padded_instance():
    """the weighted instance of the 4-wide kernel at A = 3"""
    from tests.test_gpu_prioritized_replay import _per_step_against_f64_oracle
    path = _per_step_against_f64_oracle(PIX, 32, 300, probe=True, action_dim=3)
    print("DDPG prioritized A=3: path %s" % path)
    assert path == "heads+pre"


def test_stale_nan_in_lds_does_not_reach_the_target_actor():
    """heads.hip's folded layer walks its inputs in steps of 4 up to n1ap = n1a rounded up to 4.  At n1a = 97 it reads rows 98 and
    99 of [W2; b2] (times a zero input); those must be zeros in LDS, not whatever an earlier kernel left behind the weight image --
    0 * NaN is NaN.  The LDS of every CU is first filled with NaN by matrix products of NaN matrices on the same device (torch, in
    a process of its own: it does not initialise the device in one where the library already has)."""
    import subprocess
    import sys
    code = ("import torch\n"
            "x = torch.full((8192, 8192), float('nan'), device='cuda')\n"
            "for dt in (torch.float32, torch.bfloat16, torch.float16):\n"
            "    y = x.to(dt) @ x.to(dt)\n"
            "torch.cuda.synchronize()\n"
            "assert torch.isnan(y).all()\n"
            "print('poisoned')\n")

    def poison():
        r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0 and b"poisoned" in r.stdout, r.stdout.decode()[-2000:]

    rep = _ddpg_case([100, 97, 50], "heads+pre", B=256, before_step=poison)
    assert np.isfinite(rep["err_td"]) and np.isfinite(rep["err_q"])


# ---- NAF, shared trunk.  naf_mlp_kernel: exactly two hidden layers, n0 <= 103, rep <= 51, A <= 4, B <= 1024; naf_heads_kernel:
# rep <= 63, A <= 4, B <= 16384; else GEMM levels + naf_head_kernel (A <= 8)
NAF = [
    pytest.param([100, 50], 2, 16, "mlp", id="100-50-defaults"),
    pytest.param([103, 51], 2, 16, "mlp", id="103-51-mlp-limits"),
    pytest.param([104, 50], 2, 16, "heads", id="104-50-one-past-n0"),
    pytest.param([100, 52], 2, 16, "heads", id="100-52-one-past-rep"),
    pytest.param([100, 63], 2, 16, "heads", id="100-63-K-64"),
    pytest.param([100, 64], 2, 16, "gemm", id="100-64-K-65"),
    pytest.param([50], 2, 16, "heads", id="50-one-layer"),
    pytest.param([64], 2, 16, "gemm", id="64-one-layer-K-65"),
    pytest.param([100, 100, 50], 2, 16, "heads", id="100-100-50"),
    pytest.param([1, 1], 2, 16, "mlp", id="1-1"),
    pytest.param([100, 50], 1, 16, "mlp", id="A1"),
    pytest.param([100, 50], 3, 16, "mlp", id="A3"),
    pytest.param([100, 50], 4, 16, "mlp", id="A4"),
    pytest.param([100, 50], 5, 16, "gemm", id="A5"),
    pytest.param([100, 50], 8, 16, "gemm", id="A8"),
    pytest.param([100, 50], 2, 1024, "mlp", id="B1024"),
    pytest.param([100, 50], 2, 1025, "heads", id="B1025"),
]


@pytest.mark.parametrize("hidden,A,B,path", NAF)
def test_naf_shared_trunk(hidden, A, B, path):
    from tests.test_gpu_naf import naf_fused_step_against_f64_oracle
    got = naf_fused_step_against_f64_oracle(PIX, B, True, rows=max(300, 2 * B), probe=True, hidden=hidden, action_dim=A)
    print("NAF shared hidden %s A=%d B=%d: path %s" % (hidden, A, B, got))
    assert got == path


def test_naf_own_trunks():
    from tests.test_gpu_naf import naf_fused_step_against_f64_oracle
    assert naf_fused_step_against_f64_oracle(PIX, 16, False, rows=300, probe=True, hidden=[32, 16]) == "gemm"


def test_naf_prioritized_replay_at_three_actions():
    from tests.test_gpu_naf_prioritized_replay import per_naf_step_against_f64_oracle
    assert per_naf_step_against_f64_oracle(PIX, 32, True, rows=300, probe=True, action_dim=3) == "mlp"


# ---- refusals: a Python error that names the limit, when the agent is built; the context serves a default agent afterwards
def _naf_agent(**kw):
    from tests.test_gpu_naf import make_naf
    return make_naf(PIX, 4, True, **kw)[0]


def _ddpg_agent(**kw):
    return make_pair(PIX, 4, True, **kw)[0]


@pytest.mark.parametrize("build,kw,err,msg", [
    (_naf_agent, dict(action_dim=9), RuntimeError, r"action_dim 9 outside \[1, 8\]"),
    (_ddpg_agent, dict(actor_hidden=[16] * 9), ValueError, r"9 hidden layers, at most 8"),
    (_naf_agent, dict(hidden=[16] * 9), ValueError, r"9 hidden layers, at most 8"),
    (_ddpg_agent, dict(actor_hidden=[100, 0, 50]), RuntimeError, r"hidden layer 1 has width 0 \(at least 1\)"),
    (_ddpg_agent, dict(action_dim=17), RuntimeError, r"action_dim 17 outside \[1, 16\]"),
], ids=["naf-A9", "ddpg-nine-layers", "naf-nine-layers", "zero-width", "ddpg-A17"])
def test_refusals_name_the_limit_and_leave_the_context_usable(build, kw, err, msg):
    from cartpoleplusplus_amd import _lib
    ctx = _lib.default_context()
    ctx.sync()
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        with pytest.raises(err, match=msg):
            build(**kw)
        ctx.sync()
    finally:
        ctx.prof_enable(False)
    launched = ctx.prof_read()
    assert not set(launched) & {"gemm", "heads", "naf_head", "td"}, launched
    agent = _ddpg_agent()
    try:
        agent.replay_memory.fill_synthetic(40, seed=1)
        agent.train_step(4, 2)
        agent.actor.ctx.sync()
        assert np.isfinite(agent.actor.get_params()).all() and np.isfinite(agent.critic.get_params()).all()
    finally:
        agent.close()
