"""Target policy smoothing (TD3, Fujimoto et al. 2018, section 5.3) restated in numpy: the noise the device draws
(include/cartpolepp_abi.h, cpp_ddpg_set_target_smoothing) and the critic's gradients with it.  No tests here: tests/test_tps_host.py
and tests/test_gpu_target_smoothing.py share these.

    (x, y, _, _) = philox4x32_10({b, 0x100 + i, n_lo, n_hi}, key = (seed_lo, seed_hi))
    u1 = ((x >> 8) + 1) 2^-24,  u2 = (y >> 8) 2^-24,  z = sqrt(-2 log u1) cos(2 pi u2)
    eps = clamp(sigma z, -c, c),  a' = clamp(mu'(s2) + eps, -1, 1)

FAULTS: the planted faults of the sensitivity test, each a switch of target_noise or of SmoothedDDPG.critic_gradients."""
import numpy as np

from oracle import ddpg_np as O
from tests.helpers import philox4x32_10_np

NOISE_FAULTS = ("noise_unclipped", "one_draw_for_all_rows", "one_draw_for_all_components", "n_not_advancing", "sigma_after_clip")
ORACLE_FAULTS = ("action_not_clamped", "noise_on_online_critic")
FAULTS = NOISE_FAULTS + ORACLE_FAULTS
Z_BAR = 4e-6          # |z_f32 - z_f64| before the clip: numpy's f32 evaluation measures 1.6e-6; 2.5x for a 2-ulp logf / cosine on the device


def standard_normals(seed, n, B, A, dtype=np.float64, fault=None):
    """the (B, A) pre-clip draws z of minibatch number n"""
    seed, n = int(seed), int(n)
    if fault == "n_not_advancing":
        n = 0
    b = np.repeat(np.arange(B, dtype=np.uint64), A)
    i = np.tile(np.arange(A, dtype=np.uint64), B)
    if fault == "one_draw_for_all_rows":
        b = np.zeros_like(b)
    if fault == "one_draw_for_all_components":
        i = np.zeros_like(i)
    x, y, _z, _w = philox4x32_10_np(b, np.uint64(0x100) + i, np.full_like(b, n & 0xFFFFFFFF), np.full_like(b, n >> 32),
                                    seed & 0xFFFFFFFF, seed >> 32)
    dt = np.dtype(dtype).type
    u1 = (((x >> np.uint64(8)) + np.uint64(1)).astype(dtype) * dt(2.0 ** -24)).astype(dtype)      # (0, 1]: exact in f32
    u2 = ((y >> np.uint64(8)).astype(dtype) * dt(2.0 ** -24)).astype(dtype)                        # [0, 1): exact in f32
    z = (np.sqrt(dt(-2.0) * np.log(u1)) * np.cos(dt(2.0 * np.pi) * u2)).astype(dtype)
    return z.reshape(B, A)


def target_noise(seed, n, B, A, sigma, clip, dtype=np.float64, fault=None):
    """the (B, A) clipped noise eps of minibatch number n"""
    dt = np.dtype(dtype).type
    z = standard_normals(seed, n, B, A, dtype, fault)
    if fault == "noise_unclipped":
        return (dt(sigma) * z).astype(dtype)
    if fault == "sigma_after_clip":
        return (dt(sigma) * np.clip(z, -dt(clip), dt(clip))).astype(dtype)
    return np.clip(dt(sigma) * z, -dt(clip), dt(clip)).astype(dtype)


class SmoothedDDPG(O.DDPG):
    """oracle.DDPG whose critic target is evaluated at a' = clip(mu'(s2) + noise, -1, 1)"""

    def critic_gradients(self, batch, noise=None, training=True, td_override=None, fault=None):
        """oracle.DDPG.critic_gradients (ddpg_cartpole.py:199-214) restated, with the (B, A) `noise` in front of the target critic.
        Besides the parent's outputs: 'smoothed_actions' and 'target_dq_da', dQ'/da' at the smoothed action."""
        s1, a, r, mask, s2 = batch
        dt = self.dt
        w2 = self._white(self.target_actor, s2)
        ta = self.target_actor.forward(s2, white=w2, training=training)
        fed = np.asarray(a, dt)
        sm = ta["out"]
        if noise is not None:
            if fault == "noise_on_online_critic":
                fed = (fed + np.asarray(noise, dt)).astype(dt)
            else:
                sm = (ta["out"] + np.asarray(noise, dt)).astype(dt)
                if fault != "action_not_clamped":
                    sm = np.clip(sm, dt(-1.0), dt(1.0))
        tq = self.target_critic.forward(s2, action=sm, white=w2, training=training)
        _, tdq = self.target_critic.backward(tq, np.ones_like(tq["out"]), params=False)
        y = np.asarray(r, dt) + np.asarray(mask, dt) * dt(self.hp.discount) * tq["out"]
        cb = self.critic.forward(s1, action=fed, training=training)
        td = cb["out"] - y
        B = td.shape[0]
        loss = (td * td).mean(dtype=dt)
        td_back = td if td_override is None else np.asarray(td_override, dt).reshape(td.shape)
        grads, _ = self.critic.backward(cb, (dt(2.0) * td_back / dt(B)).astype(dt))
        return {"q": cb["out"], "td": td, "loss": loss, "target_q": tq["out"], "target_actions": ta["out"],
                "smoothed_actions": sm, "target_dq_da": tdq, "cache_critic": cb,
                "grads": O.flatten(self.critic.spec, grads, self.dt)}


def td_bar(discount, sigma, target_dq_da, atol=1e-5):
    """how far a device TD may sit from the float64 one: the suite's bar plus the propagated noise bar -- a draw Z_BAR * sigma away
    moves Q' by at most that times sum_i |dQ'/da'_i| (first order; the clamps only shrink it), and TD by discount times that"""
    return atol + float(discount) * Z_BAR * float(sigma) * float(np.abs(np.asarray(target_dq_da, np.float64)).sum(axis=1).max())


# ---- the cases tests/test_gpu_target_smoothing.py holds to SmoothedDDPG(float64), shared with the CPU-only sensitivity test
# (tests.helpers.host_case(shape, B, 1, host_seed, rows, action_dim): the same parameters, episodes and rows)
CASE_SHAPE, CASE_ROWS = (16, 16, 3, 1, 2), 300
SIGMA, CLIP, NOISE_SEED = 0.5, 0.5, 0x5EEDF00D12345
# name: (B, A, host_case seed, n of the checked minibatch)
ORACLE_CASES = {"A2": (16, 2, 11, 1), "A9": (16, 9, 12, 1)}
SATURATED_BIAS = 2.0          # tanh(2) = 0.964: noise beyond 0.036 in that direction crosses the +-1 clamp


def saturate_target_actor(flat, aspec):
    """the target actor's parameter vector with the output layer's bias at +SATURATED_BIAS on component 0 and -SATURATED_BIAS on
    component 1 and the weights into those two components scaled down, so that tanh sits near +-0.96 there"""
    flat = np.array(flat, np.float32)
    off = 0
    last_w = last_b = None
    for name, shp in aspec.layout():
        n = int(np.prod(shp))
        if name.endswith("/weights") and len(shp) == 2:
            last_w = (off, shp)
        if name.endswith("/biases"):
            last_b = (off, shp)
        off += n
    (wo, wshp), (bo, _bshp) = last_w, last_b
    W = flat[wo:wo + int(np.prod(wshp))].reshape(wshp)
    W[:, :2] *= np.float32(0.05)
    flat[bo + 0], flat[bo + 1] = SATURATED_BIAS, -SATURATED_BIAS
    return flat
