"""fp64 references, per-element rounding bounds, an fp32 restatement and the shared case tables of the optimizer kernels
(csrc/nrv_optim.hip: nrv_sumsq_f32, nrv_adamw_f32).  Host only (numpy); tests/test_optim_ref_host.py proves the bounds on the
restatement and shows that each of MISTAKES breaks them; tests/test_optim_edges_gpu.py and tests/test_fused_adamw_gpu.py judge the
kernels and optim.FusedAdamW with them.

The reference (`adamw_ref`) is clip_grad_norm_ followed by torch.optim.AdamW in float64:
    coef = min(1, max_norm / (sqrt(gnorm_sq) + 1e-6))       (1 when max_norm <= 0 or no norm is given; NaN stays NaN)
    g'   = coef g;   p1 = p (1 - lr wd);   m' = b1 m + (1 - b1) g';   v' = b2 v + (1 - b2) g' g'
    p'   = p1 - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
`gnorm_sq` is the fp32 number the kernel reads, so the error of the norm is not part of these bounds (`sumsq_ref` has its own).
The hyper-parameters are rounded where the C entry rounds them: lr, b1, b2, eps to fp32; decay = 1 - lr wd, omb = 1 - b,
step_size = lr / (1 - b1^t) and inv_bc2_sqrt = 1 / sqrt(1 - b2^t) are computed in double and then rounded; max_norm is an fp32
argument.  round_hyper=False keeps them in double (the comparison with torch.optim.AdamW on float64 tensors).

Bounds.  u = 2^-24 is the unit round-off of fp32: one rounding of x costs at most u |x|, or Q / 2 with Q = 2^-149 (the subnormal
quantum) where x is subnormal.  The operation sequence of `adamw_one`, hats for the float64 values:
    coef     sqrtf, the add of 1e-6f (itself 1e-6 rounded: the reference adds 1e-6), the divide      relative KC u, KC = 4
             (0 where nothing is clipped by construction: max_norm <= 0).  min(1, .) is a contraction, so the bound holds on
             either side of the clamp.
    g1       = fl(g coef)                                   relative (KC + 1) u
    m'       = fmaf(b1, m, fl(omb1 g1))                     m_bound = u ((KC + 3) |omb1 g'| + |b1 m|) + Q
                                                            (g1, the product, the share of the fma's rounding; the fma's on b1 m)
    v'       = fmaf(b2, v, fl(fl(omb2 g1) g1))              v_bound = u ((2 KC + 5) |omb2 g'^2| + |b2 v|) + 2 Q
                                                            (g1 twice, two products, the fma)
    s        = sqrtf(v')                                    es = sqrt(v') - sqrt(max(v' - v_bound, 0)) + u s   (sqrt is concave: the
                                                            step down is the larger one; no division by a vanishing v')
    d        = fmaf(s, inv_bc2_sqrt, eps)                   ed = inv_bc2_sqrt es + u d
    q        = m' / d                                       eq = m_bound / (d - ed) + |q| ed / (d - ed) + u |q| + Q
    p'       = fl(fl(p decay) - fl(step_size q))            p_bound = u (|p decay| + |step_size q| + |p'|) + step_size eq + 2 Q
The compiler may contract the last line into fmaf(-step_size, q, fl(p decay)) or fmaf(p, decay, -fl(step_size q)); each drops
one of the three roundings the bound counts, so the bound covers the plain form and both contractions (`restated(contract=)`
states all three).  Every k is the count of the sequence above and the terms are first order in u.  Over the whole table the
restatement's error / bound has a median near 0.2 and a worst of 0.99 (printed by the host test).  The worst sits where the
bound is one or two roundings and nothing else -- an element whose gradient is zero has the ONE rounding of fmaf(b, x, 0) as
its m and v bound, and |p| just above a power of two makes u |p| the full half-ulp of both roundings of the last line -- and a
single rounding cannot exceed u |x|; the higher orders are 2^-23 of the bound.

sumsq.  The kernels add in a fixed tree: every thread an fma chain over its elements (the square is inside the fma: no rounding
of its own), a six-step butterfly over the wave, the four wave sums, and the same again over the per-block partials.  An
addend passes at most `sumsq_depth(n)` additions, so |error| <= (depth + SUMSQ_SLACK) u sum(x^2) + depth Q.
"""
from __future__ import annotations

import math
import zlib

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
Q = 2.0 ** -149
KC = 4
THREADS = 256                    # OPT_THREADS
SUMSQ_BLOCKS = 1024              # the cap of nrv_sumsq_f32
SUMSQ_SLACK = 2


def _rng(*key) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def to_bf16(x: np.ndarray) -> np.ndarray:
    """fp32 values rounded to bf16 (nearest even), kept as fp32"""
    b = np.ascontiguousarray(x, dtype=f32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(f32)


def ratio(got, ref, bound) -> float:
    """max over the elements of |got - ref| / bound (0 / 0 counts as 0); a non-finite result counts as inf"""
    got, ref, bound = (np.asarray(a, dtype=f64).reshape(-1) for a in (got, ref, bound))
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


# ----------------------------------------------------------------------------------------------
# AdamW
# ----------------------------------------------------------------------------------------------
def host_scalars(lr, beta1, beta2, eps, weight_decay, t, rounded=True, beta_pow_step=None, omb2_in_float=False):
    """The scalars of AdamWArgs as nrv_adamw_f32 computes them (double, then one rounding to fp32)"""
    r = (lambda x: float(f32(x))) if rounded else float
    tt = float(t if beta_pow_step is None else beta_pow_step)
    bc1 = 1.0 - math.pow(beta1, tt)
    bc2 = 1.0 - math.pow(beta2, tt)
    with np.errstate(divide="ignore"):
        step_size = float(f64(lr) / f64(bc1))
        inv_bc2_sqrt = float(f64(1.0) / np.sqrt(f64(bc2)))
    omb2 = float(f32(1.0) - f32(beta2)) if omb2_in_float else r(1.0 - beta2)
    return dict(lr=r(lr), beta1=r(beta1), beta2=r(beta2), eps=r(eps), decay=r(1.0 - lr * weight_decay),
                omb1=r(1.0 - beta1), omb2=omb2, step_size=r(step_size), inv_bc2_sqrt=r(inv_bc2_sqrt))


def clip_coef(gnorm_sq, max_norm, rounded=True) -> float:
    """float64 clip_grad_norm_ coefficient from the (fp32) sum of squares and the (fp32) max_norm; NaN propagates"""
    max_norm = float(f32(max_norm)) if rounded else float(max_norm)
    if gnorm_sq is None or not max_norm > 0.0:
        return 1.0
    with np.errstate(invalid="ignore"):
        c = f64(max_norm) / (np.sqrt(f64(gnorm_sq)) + 1e-6)
    return float(np.minimum(c, 1.0))                     # np.minimum hands a NaN on


def adamw_ref(p, g, m, v, lr, beta1, beta2, eps, weight_decay, t, gnorm_sq=None, max_norm=0.0, round_hyper=True) -> dict:
    """One step in float64 and the per-element bounds of the module docstring: {p, m, v, p_bound, m_bound, v_bound}"""
    h = host_scalars(lr, beta1, beta2, eps, weight_decay, t, rounded=round_hyper)
    p, g, m, v = (np.asarray(a, dtype=f64) for a in (p, g, m, v))
    coef = clip_coef(gnorm_sq, max_norm, rounded=round_hyper)
    kc = KC if (gnorm_sq is not None and float(f32(max_norm)) > 0.0) else 0
    with np.errstate(invalid="ignore", over="ignore"):
        g1 = g * coef
        p1 = p * h["decay"]
        mg, mm = h["omb1"] * g1, h["beta1"] * m
        m2 = mm + mg
        vg, vv = h["omb2"] * g1 * g1, h["beta2"] * v
        v2 = vv + vg
        s = np.sqrt(v2)
        d = s * h["inv_bc2_sqrt"] + h["eps"]
        q = m2 / d
        upd = h["step_size"] * q
        p2 = p1 - upd
        m_bound = U * ((kc + 3) * np.abs(mg) + np.abs(mm)) + Q
        v_bound = U * ((2 * kc + 5) * np.abs(vg) + np.abs(vv)) + 2 * Q
        es = s - np.sqrt(np.maximum(v2 - v_bound, 0.0)) + U * s
        ed = h["inv_bc2_sqrt"] * es + U * d
        eq = m_bound / (d - ed) + np.abs(q) * ed / (d - ed) + U * np.abs(q) + Q
        p_bound = U * (np.abs(p1) + np.abs(upd) + np.abs(p2)) + h["step_size"] * eq + 2 * Q
    return dict(p=p2, m=m2, v=v2, p_bound=p_bound, m_bound=m_bound, v_bound=v_bound, coef=coef)


def _fma32(a, b, c):
    """fmaf: the float64 multiply-add rounded once to fp32"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, dtype=f64) * np.asarray(b, dtype=f64) + np.asarray(c, dtype=f64)).astype(f32)


MISTAKES = ("omb2_in_float", "eps_before_bias_correction", "decay_after_update", "bias_correction_of_previous_step",
            "clip_without_1e-6", "clip_not_clamped", "v_from_unclipped_gradient", "tail_unclipped", "bf16_halves_swapped",
            "decay_on_moment")
CONTRACTIONS = (None, "decay", "update")


def restated_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, t, gnorm_sq, max_norm, bf16_grad=False, mistake=None,
                  contract=None):
    """`adamw_kernel` / `adamw_one` in fp32 on the CPU, in the kernel's order: (p, m, v) as fp32 arrays.  `contract`: None, or
    which product the compiler fuses into the final subtraction ("decay": fmaf(p, decay, -fl(step_size q)); "update":
    fmaf(-step_size, q, fl(p decay))).  `mistake`: one name of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    assert contract in CONTRACTIONS
    h = host_scalars(lr, beta1, beta2, eps, weight_decay, t, omb2_in_float=(mistake == "omb2_in_float"),
                     beta_pow_step=(t - 1 if mistake == "bias_correction_of_previous_step" else None))
    h = {k: f32(x) for k, x in h.items()}
    p, g, m, v = (np.array(a, dtype=f32).reshape(-1) for a in (p, g, m, v))
    n = p.size
    if mistake == "bf16_halves_swapped" and bf16_grad:
        body = g[:n // 4 * 4].reshape(-1, 2)[:, ::-1].reshape(-1)
        g = np.concatenate((body, g[n // 4 * 4:]))
    one = f32(1.0)
    coef = np.full(n, one, dtype=f32)
    mx = f32(max_norm)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        if gnorm_sq is not None and mx > 0:
            nrm = np.sqrt(f32(gnorm_sq))
            c = mx / (nrm if mistake == "clip_without_1e-6" else nrm + f32(1e-6))
            if mistake != "clip_not_clamped":
                c = c if not (c >= one) else one
            coef[:] = c
            if mistake == "tail_unclipped":
                coef[n // 4 * 4:] = one
        g1 = g * coef
        gv = g if mistake == "v_from_unclipped_gradient" else g1
        m2 = _fma32(h["beta1"], m, h["omb1"] * g1)
        if mistake == "decay_on_moment":
            m2 = m2 * h["decay"]
        v2 = _fma32(h["beta2"], v, (h["omb2"] * gv) * gv)
        s = np.sqrt(v2)
        if mistake == "eps_before_bias_correction":
            d = (s + h["eps"]) * h["inv_bc2_sqrt"]
        else:
            d = _fma32(s, h["inv_bc2_sqrt"], h["eps"])
        q = m2 / d
        if mistake == "decay_after_update":
            p2 = (p - h["step_size"] * q) * h["decay"]
        elif mistake == "decay_on_moment":
            p2 = p - h["step_size"] * q
        elif contract == "decay":
            p2 = _fma32(p, h["decay"], -(h["step_size"] * q))
        elif contract == "update":
            p2 = _fma32(-h["step_size"], q, p * h["decay"])
        else:
            p2 = p * h["decay"] - h["step_size"] * q
    assert p2.dtype == f32 and m2.dtype == f32 and v2.dtype == f32
    return p2, m2, v2


# ---- the case table ----------------------------------------------------------------------------
LENGTHS = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 4 * 256 * 3 + 1)
SUMSQ_LENGTHS = LENGTHS + (1048576 + 7,)         # the first size at which the 1024-block cap gives a thread a second pass
STEPS = (1, 2, 10, 1000, 100000)
KINDS = ("random_1", "random_1e-3", "random_1e-6", "tiny", "zeros_with_state", "spike_tail")
HYPERS = {"trainer": (3e-3, 0.9, 0.999, 1e-8, 0.05), "no_decay": (3e-3, 0.9, 0.999, 1e-8, 0.0),
          "big_eps": (3e-3, 0.9, 0.999, 1e-3, 0.05), "zero_betas": (3e-3, 0.0, 0.0, 1e-8, 0.05)}
CLIPS = ("none", "above", "below", "edge")
GRAD_DTYPES = ("f32", "bf16")
SWEEP_N = 4 * 256 * 3 + 1                        # three blocks and a tail element: the length of the hyper-parameter sweep
_SCALE = {"random_1": 1.0, "random_1e-3": 1e-3, "random_1e-6": 1e-6, "tiny": 1e-10, "zeros_with_state": 1e-2, "spike_tail": 1.0}


def gradient(kind, n, key):
    r = _rng("g", kind, n, key)
    if kind.startswith("random"):
        return (r.standard_normal(n) * _SCALE[kind]).astype(f32)
    if kind == "tiny":               # 1e-12 <= |g| <= 1e-8: sqrt(v) near eps = 1e-8, g^2 >= 1e-24 far above the fp32 underflow threshold
        return (np.sign(r.standard_normal(n)) * 10.0 ** r.uniform(-12.0, -8.0, n)).astype(f32)
    if kind == "zeros_with_state":
        g = (r.standard_normal(n) * _SCALE[kind]).astype(f32)
        g[::3] = 0.0
        return g
    if kind == "spike_tail":         # all the energy in the elements the scalar tail loop handles
        g = np.zeros(n, dtype=f32)
        k = n % 4
        g[n - k:] = (np.sign(r.standard_normal(k)) * (1.0 + r.uniform(0.0, 1.0, k))).astype(f32)
        return g
    raise ValueError(kind)


class Case:
    """One call of nrv_adamw_f32: inputs, hyper-parameters, the fp32 sum of squares it reads and max_norm"""
    def __init__(self, n, kind, t, hyper, clip, gdt):
        self.n, self.kind, self.t, self.hyper, self.clip, self.gdt = n, kind, t, hyper, clip, gdt
        self.name = f"{kind}-n{n}-t{t}-{hyper}-{clip}-{gdt}"
        self.lr, self.beta1, self.beta2, self.eps, self.wd = HYPERS[hyper]

    def __repr__(self):
        return self.name

    def arrays(self):
        """p, g, m, v (fp32; g holds bf16 values when the case's gradients are bf16), gnorm_sq (fp32 or None), max_norm (fp32)"""
        key = (self.t, self.hyper, self.clip)
        r = _rng("state", self.kind, self.n, key)
        p = r.standard_normal(self.n).astype(f32)
        g = gradient(self.kind, self.n, key)
        if self.gdt == "bf16":
            g = to_bf16(g)
        sc = _SCALE[self.kind] if self.kind != "spike_tail" else 1e-2
        if self.t == 1 and self.kind != "zeros_with_state":
            m, v = np.zeros(self.n, dtype=f32), np.zeros(self.n, dtype=f32)
        else:
            m = (r.standard_normal(self.n) * sc * 0.5).astype(f32)
            v = ((r.standard_normal(self.n) * sc) ** 2).astype(f32)
        gn = f32((g.astype(f64) ** 2).sum())
        norm = math.sqrt(float(gn))
        if self.clip == "none":
            return p, g, m, v, None, f32(0.0)
        if self.clip == "above":
            mx = f32(max(norm, 1e-30) * 64.0 + 1e-4)               # the coefficient must be exactly 1
        elif self.clip == "below":
            mx = f32(norm / 37.0)
        else:                                                       # the quotient within a few ulps of 1, on either side
            k = int(r.integers(-3, 4))
            mx = f32(f32(norm + 1e-6) * f32(1.0 + k * 2.0 ** -23))
        return p, g, m, v, gn, mx

    def ref(self):
        p, g, m, v, gn, mx = self.arrays()
        return adamw_ref(p, g, m, v, self.lr, self.beta1, self.beta2, self.eps, self.wd, self.t, gn, float(mx))

    def args(self):
        return (self.lr, self.beta1, self.beta2, self.eps, self.wd, self.t)


def restated(case: Case, mistake=None, contract=None):
    p, g, m, v, gn, mx = case.arrays()
    return restated_step(p, g, m, v, *case.args(), gn, mx, bf16_grad=(case.gdt == "bf16"), mistake=mistake, contract=contract)


def _cases():
    out, seen = [], set()

    def add(n, kind, t, hyper, clip, gdt):
        if kind == "spike_tail" and n % 4 == 0:          # no tail to put the energy in
            return
        c = Case(n, kind, t, hyper, clip, gdt)
        if c.name not in seen:
            seen.add(c.name)
            out.append(c)

    hy = list(HYPERS)
    # every length with every gradient kind and both gradient types; the other axes cycle with strides that do not divide each other
    i = 0
    for n in LENGTHS:
        for kind in KINDS:
            for gdt in GRAD_DTYPES:
                add(n, kind, STEPS[i % 5], hy[(i // 2) % 4], CLIPS[(i // 3 + i) % 4], gdt)
                i += 1
    # every step, hyper-parameter set, max_norm and gradient kind with each other, at three blocks and a tail element
    for t in STEPS:
        for hyper in hy:
            for clip in CLIPS:
                for kind in KINDS:
                    add(SWEEP_N, kind, t, hyper, clip, "f32")
    # bf16 gradients clipped at every length (the vector body and the scalar tail read them through different loads)
    for n in LENGTHS:
        add(n, "random_1e-3", 2, "trainer", "below", "bf16")
    return out


CASES = _cases()
CASE_BY_NAME = {c.name: c for c in CASES}


# ----------------------------------------------------------------------------------------------
# sum of squares
# ----------------------------------------------------------------------------------------------
def sumsq_blocks(n: int) -> int:
    """the grid of sumsq_partial_kernel as nrv_sumsq_f32 sizes it"""
    n4 = n // 4
    return max(1, min((n4 + THREADS - 1) // THREADS, SUMSQ_BLOCKS))


def sumsq_depth(n: int) -> int:
    """the largest number of additions an addend passes in the fixed tree"""
    n4, blocks = n // 4, sumsq_blocks(n)
    chain = -(-n4 // (blocks * THREADS)) * 4 + (1 if n % 4 else 0)
    final = -(-blocks // THREADS)
    return chain + 6 + 4 + final + 6 + 4


def sumsq_ref(x):
    """(float64 sum of squares, bound)"""
    x = np.asarray(x, dtype=f64).reshape(-1)
    s = float((x * x).sum())
    d = sumsq_depth(x.size)
    return s, (d + SUMSQ_SLACK) * U * s + d * Q


def _block_sum(s):
    """[blocks, 256] per-thread values -> per-block value: butterfly over each wave, then the four wave sums in order"""
    w = s.reshape(-1, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, lane ^ o]).astype(f32)
    red = w[:, 0].reshape(-1, THREADS // 64)
    t = np.zeros(red.shape[0], dtype=f32)
    for k in range(THREADS // 64):
        t = (t + red[:, k]).astype(f32)
    return t


def sumsq_restated(x, omit_tail=False) -> float:
    """sumsq_partial_kernel + sumsq_final_kernel in fp32 on the CPU, in the kernels' order"""
    x = np.asarray(x, dtype=f32).reshape(-1)
    n = x.size
    n4, blocks = n // 4, sumsq_blocks(n)
    T = blocks * THREADS
    s = np.zeros(T, dtype=f32)
    body = x[:4 * n4].reshape(n4, 4)
    for lo in range(0, n4, T):                          # one grid-stride pass: thread i takes the vector lo + i
        cnt = min(T, n4 - lo)
        for e in range(4):
            ve = body[lo:lo + cnt, e]
            s[:cnt] = _fma32(ve, ve, s[:cnt])
    if not omit_tail:
        tail = x[4 * n4:]                               # block 0, thread i takes element 4 n4 + i (fewer than 4 of them)
        s[:tail.size] = _fma32(tail, tail, s[:tail.size])
    partial = _block_sum(s.reshape(blocks, THREADS))
    fs = np.zeros(THREADS, dtype=f32)
    for lo in range(0, blocks, THREADS):
        cnt = min(THREADS, blocks - lo)
        fs[:cnt] = (fs[:cnt] + partial[lo:lo + cnt]).astype(f32)
    return float(_block_sum(fs.reshape(1, THREADS))[0])


SUMSQ_KINDS = ("random_1", "random_1e-3", "random_1e-6", "tiny", "zeros_with_state", "spike_tail", "ones")
SUMSQ_CASES = [(n, kind, gdt) for n in SUMSQ_LENGTHS for kind in SUMSQ_KINDS for gdt in GRAD_DTYPES
               if not (kind == "spike_tail" and n % 4 == 0)]


def sumsq_input(n, kind, gdt):
    x = np.ones(n, dtype=f32) if kind == "ones" else gradient(kind, n, "sumsq")
    return to_bf16(x) if gdt == "bf16" else x


def edge_indices(n):
    """where the loops of the kernels begin and end: the first vector, the last thread of block 0 and the first of block 1, the
    last vector element, each tail element, the last element"""
    n4 = n // 4
    idx = {0, 3, 4 * THREADS - 1, 4 * THREADS, 4 * n4 - 1, n - 1} | set(range(4 * n4, n))
    return sorted(i for i in idx if 0 <= i < n)


def edge_powers(n):
    """zeros except distinct powers of two at edge_indices(n): the sum of squares is exact in fp32 (and the values in bf16)"""
    x = np.zeros(n, dtype=f32)
    for k, i in enumerate(edge_indices(n)):
        x[i] = 2.0 ** (k - 4)
    return x
