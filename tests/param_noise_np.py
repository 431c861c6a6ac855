"""Parameter-space exploration noise (Plappert et al. 2018) restated in numpy: what a resample of the device does
(include/cartpolepp_abi.h, cpp_ddpg_set_param_noise), the bars the device is held to, and the planted faults that must leave them.  No
tests here: tests/test_param_noise_host.py and tests/test_gpu_param_noise.py share these.

    (x, y, _, _) = philox4x32_10({i, 0x200, n_lo, n_hi}, key = (seed_lo, seed_hi))          i: the element of the flat parameter buffer
    u1 = ((x >> 8) + 1) 2^-24,  u2 = (y >> 8) 2^-24,  z = sqrt(-2 log u1) cos(2 pi u2)       (no clip)
    pt[i] = fma(sigma, z_i, p[i])  for i < n_noise;   pt[i] = p[i]  behind it (the feature layer norm's gamma and beta)
    d = sqrt(sum_{b,k} (a[b][k] - at[b][k])^2 / (B A));   sigma' = sigma * alpha if d < delta else sigma / alpha;   n' = n + 1

A resample draws with the sigma and the n it finds, measures the copy it has just drawn, and leaves sigma' and n' for the NEXT one.

FAULTS: each a switch of one function below.  RATIOS: the comparison functions -- each returns (error / bar); a value above 1 has left
its bar, and the GPU test asserts that none does."""
import numpy as np

from tests.helpers import philox4x32_10_np
from tests.tps_np import Z_BAR

FAULTS = ("layer_norm_perturbed",            # gamma and beta take noise like every other element
          "n_not_advancing",                 # every resample draws at n = 0
          "one_draw_for_all_elements",       # the Philox counter's word 0 is 0 for every element
          "index_mod_2_16",                  # ... or the element index modulo 2^16
          "n_hi_ignored",                    # word 3 is 0: n = 2^32 draws what n = 0 drew
          "sum_not_mean",                    # d = sqrt(sum) without the division by B A
          "no_square_root",                  # d = the mean square
          "adapt_inverted",                  # sigma grows when the distance is above the target
          "adapt_on_current_copy",           # the copy is drawn again with the adapted sigma instead of the one it was measured with
          "sigma_twice")                     # pt = p + sigma (sigma z)
STREAM = 0x200


def normals(seed, n, count, dtype=np.float64, fault=None, first=0):
    """z of elements [first, first + count) of draw number n"""
    seed, n = int(seed), int(n)
    i = np.arange(first, first + count, dtype=np.uint64)
    assert first + count <= 1 << 32
    if fault == "n_not_advancing":
        n = 0
    if fault == "one_draw_for_all_elements":
        i = np.zeros_like(i)
    if fault == "index_mod_2_16":
        i = i & np.uint64(0xFFFF)
    n_hi = 0 if fault == "n_hi_ignored" else n >> 32
    x, y, _z, _w = philox4x32_10_np(i, np.full_like(i, STREAM), np.full_like(i, n & 0xFFFFFFFF), np.full_like(i, n_hi), seed & 0xFFFFFFFF, seed >> 32)
    dt = np.dtype(dtype).type
    u1 = (((x >> np.uint64(8)) + np.uint64(1)).astype(dtype) * dt(2.0 ** -24)).astype(dtype)      # (0, 1]: exact in f32
    u2 = ((y >> np.uint64(8)).astype(dtype) * dt(2.0 ** -24)).astype(dtype)                        # [0, 1): exact in f32
    return (np.sqrt(dt(-2.0) * np.log(u1)) * np.cos(dt(2.0 * np.pi) * u2)).astype(dtype)


def perturbed(p, sigma, seed, n, n_noise, dtype=np.float64, fault=None):
    """the perturbed copy of the flat float32 vector p.  float64: p + sigma z exactly enough to be the reference; float32 (the twin): z in
    float32, the fused multiply-add formed in float64 from the float32 operands (the product is exact there) and rounded once more"""
    p = np.asarray(p, np.float32)
    dt = np.dtype(dtype).type
    z = normals(seed, n, len(p), dtype, fault).astype(np.float64)
    s = float(dt(sigma))
    step = s * (s * z) if fault == "sigma_twice" else s * z
    out = (p.astype(np.float64) + step).astype(dtype)
    if fault != "layer_norm_perturbed":
        out[int(n_noise):] = p[int(n_noise):]
    return out


def distance(a, at, dtype=np.float64, fault=None):
    a, at = np.asarray(a, np.float32).astype(np.float64), np.asarray(at, np.float32).astype(np.float64)
    sq = ((a - at) ** 2).sum(dtype=np.float64)
    if fault != "sum_not_mean":
        sq = sq / float(a.size)
    return np.dtype(dtype).type(sq if fault == "no_square_root" else np.sqrt(sq))


def adapted_sigma(sigma, d, delta, alpha, dtype=np.float64, fault=None):
    """one operation of `dtype`: float32 is the device's, to the bit (IEEE multiplication and division)"""
    dt = np.dtype(dtype).type
    grow = dt(d) < dt(delta)
    if fault == "adapt_inverted":
        grow = not grow
    return dt(dt(sigma) * dt(alpha)) if grow else dt(dt(sigma) / dt(alpha))


class Restated(object):
    """the trainer's words and one resample, as the header states it.  actions: None, or a callable (perturbed copy) -> (a, at)"""

    def __init__(self, sigma0, delta, alpha, seed, dtype=np.float64, fault=None):
        self.dtype, self.fault = dtype, fault
        dt = np.dtype(dtype).type
        self.sigma, self.delta, self.alpha, self.seed = dt(np.float32(sigma0)), np.float32(delta), np.float32(alpha), int(seed)
        self.n, self.d, self.adapted = 0, dt(0.0), False

    def resample(self, p, n_noise, actions=None):
        pt = perturbed(p, self.sigma, self.seed, self.n, n_noise, self.dtype, self.fault)
        self.adapted = actions is not None
        if actions is not None:
            a, at = actions(pt)
            self.last = (np.asarray(a, np.float32), np.asarray(at, np.float32))
            self.d = distance(a, at, self.dtype, self.fault)
            self.sigma = adapted_sigma(self.sigma, self.d, self.delta, self.alpha, self.dtype, self.fault)
            if self.fault == "adapt_on_current_copy":
                pt = perturbed(p, self.sigma, self.seed, self.n, n_noise, self.dtype, self.fault)
        if self.fault != "n_not_advancing":
            self.n += 1
        return pt


# ---- the bars.  Each function returns error / bar (inf where bits must agree and do not)
def element_bars(p, sigma, z):
    """per element: the device's z may sit Z_BAR from the float64 one (tests/tps_np.py: a 2-ulp logf and cosine), which sigma scales; the
    fused multiply-add rounds once, half an ulp of its result: 2^-24 |p + sigma z|"""
    p, z, s = np.asarray(p, np.float64), np.asarray(z, np.float64), float(np.float32(sigma))
    return s * Z_BAR + 2.0 ** -24 * np.abs(p + s * z)


def perturbation_ratio(got, p, sigma, seed, n, n_noise):
    """a perturbed copy `got` (float32, every element) against the float64 restatement drawn with (sigma, seed, n): the worst element's
    error over its bar; the elements from n_noise on must be p's, bit for bit"""
    got, p = np.asarray(got), np.asarray(p, np.float32)
    assert got.dtype == np.float32 and got.shape == p.shape and p.ndim == 1
    n_noise = int(n_noise)
    if not np.array_equal(got[n_noise:].view(np.uint32), p[n_noise:].view(np.uint32)):
        return float("inf")
    if n_noise == 0:
        return 0.0
    z = normals(seed, n, n_noise, np.float64)
    want = p[:n_noise].astype(np.float64) + float(np.float32(sigma)) * z
    bars = element_bars(p[:n_noise], sigma, z)
    err = np.abs(got[:n_noise].astype(np.float64) - want)
    if float(np.float32(sigma)) == 0.0:      # (a bit copy: fma(0, z, p) is p)
        return 0.0 if np.array_equal(got.view(np.uint32), p.view(np.uint32)) else float("inf")
    return float((err / bars).max())


def distance_bar(d, count):
    """count differences and squares in f64 (the difference of two floats is exact there, the square rounds once), count - 1 additions, a
    division, a root: relative (count + 2) 2^-53 on d however they are ordered; then one rounding to float32, 2^-24"""
    return abs(float(d)) * ((int(count) + 2) * 2.0 ** -53 + 2.0 ** -24)


def distance_ratio(got_d, a, at):
    want = float(distance(a, at, np.float64))
    bar = distance_bar(want, np.asarray(a).size)
    err = abs(float(got_d) - want)
    return (err / bar) if bar > 0 else (0.0 if err == 0 else float("inf"))


def decided(d, delta, count):
    """whether |d - delta| exceeds d's bar: the branch of the adaptation does not hang on a rounding"""
    return abs(float(d) - float(np.float32(delta))) > distance_bar(d, count)


def sigma_ratio(got_sigma, sigma_before, got_d, delta, alpha):
    """the adapted sigma against the float32 twin's, from the device's own float32 d: bits"""
    want = adapted_sigma(np.float32(sigma_before), np.float32(got_d), delta, alpha, np.float32)
    return 0.0 if np.float32(got_sigma).view(np.uint32) == np.float32(want).view(np.uint32) else float("inf")


def count_ratio(got_n, n_before):
    return 0.0 if int(got_n) == int(n_before) + 1 else float("inf")


def resample_ratios(got_pt, got_words, p, n_noise, before, seed, delta, alpha, actions=None):
    """every bar of ONE resample.  got_pt: the device's perturbed copy; got_words: its (sigma, d, n, adapted) behind the resample; before:
    (sigma, d, n) in front of it; actions: the device's own (a, at) of a measured resample, or None."""
    sigma0, d0, n0 = before
    sigma1, d1, n1, adapted = got_words
    out = {"perturbation": perturbation_ratio(got_pt, p, sigma0, seed, n0, n_noise), "count": count_ratio(n1, n0),
           "adapted_flag": 0.0 if bool(adapted) == (actions is not None) else float("inf")}
    if actions is None:
        same = np.float32(sigma1).view(np.uint32) == np.float32(sigma0).view(np.uint32) and np.float32(d1).view(np.uint32) == np.float32(d0).view(np.uint32)
        out["left_alone"] = 0.0 if same else float("inf")
    else:
        out["distance"] = distance_ratio(d1, *actions)
        out["sigma"] = sigma_ratio(sigma1, sigma0, d1, delta, alpha)
    return out


def worst(ratios):
    return max(ratios.values())
