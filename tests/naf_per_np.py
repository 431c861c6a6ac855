"""float64 reference of the weighted NAF gradient (prioritized replay: loss = mean(w td^2), dQ = (td w) 2 / B; include/cartpolepp_abi.h).
oracle.naf_np.NAF.forward_backward has no hook for dQ, so this subclass restates it with per-row weights; everything below dQ is the
parent's own code (_backward_head, _backward_value).  tests/test_naf_per_host.py proves it against the unmodified oracle."""
import numpy as np

from oracle import naf_np as N


class WeightedNAF(N.NAF):
    def forward_backward(self, batch, backward=True, w=None):
        """the parent's forward_backward with importance weights w (B,) on the rows; w None: the parent's"""
        if w is None:
            return N.NAF.forward_backward(self, batch, backward)
        s1, a, r, mask, s2 = batch
        dt, A = self.dt, self.A
        B = np.asarray(a).shape[0]
        w = np.asarray(w, dt).reshape(B, 1)
        cv, cm, cl = self._forward(s1, training=backward)
        V, mu, lv = cv["out"], cm["out"], cl["out"]
        L = N.build_L(lv, A, dt)
        d = np.asarray(a, dt) - mu
        z = np.einsum("bij,bi->bj", L, d)
        adv = (-0.5 * (z * z).sum(axis=1, keepdims=True)).astype(dt)
        q = V + adv
        tv = self.target_value.forward(s2, training=backward)["out"]
        y = np.asarray(r, dt) + np.asarray(mask, dt) * dt(self.discount) * tv
        td = q - y
        loss = (w * (td * td)).mean(dtype=dt)
        out = {"l_values": lv, "loss": loss, "value": V, "advantage": adv, "target_value": tv, "q": q, "mu": mu, "td": td,
               "finite": bool(np.isfinite(lv).all() and np.isfinite(L).all() and np.isfinite(loss))}
        if not backward:
            return out
        dq = (dt(2.0) * (td * w) / dt(B)).astype(dt)
        dz = -z * dq
        dL = np.einsum("bi,bj->bij", d, dz)
        dd = np.einsum("bij,bj->bi", L, dz)
        dl = np.zeros_like(lv)
        for i in range(A):
            off = (i * (i + 1)) // 2
            dl[:, off:off + i] = dL[:, i, :i]
            dl[:, off + i] = dL[:, i, i] * L[:, i, i]
        gl, drep_l = self._backward_head(self.l, cl, dl)
        gm, drep_m = self._backward_head(self.mu, cm, -dd)
        gv = self._backward_value(cv, dq, extra=drep_l + drep_m if self.share else None)
        out["grads"] = np.concatenate([gv, gm, gl])
        return out
