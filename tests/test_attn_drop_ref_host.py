"""CPU: tests/attn_drop_ref.py before any kernel runs -- the numpy restatement of the keep decisions (statistics, prefix property,
threshold), the kernels' rounding points against fp64 on every row of every case, the seven mistakes, the probes, and the argument
errors and declarations of the four nrv_attn_drop_* entries.

Measured here (restated(kernel_rounding=True) against fp64, worst row over the 58 cases, error / KERNEL_ROUNDING_BOUND = 1.5e-2):
o 0.25, dq 0.59, dk 0.37, dv 0.29; no case needed other inputs.  Each mistake puts at least 38 of the 58 cases over PER_ROW_BOUND on
the random inputs already (tile_local_k: the 38 cases with N > 64), and fails a probe exactly."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_drop_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_CASES = tuple(c for c in R.CASES if c.N in (1, 17, 65, 208, 257, 300) or (c.family == "stream" and c.N == 129))


def test_case_list_is_the_one_the_kernels_need():
    assert len(R.CASES) == len(R.AE.SINGLE_PASS_NS) + 4 * 6 + 2
    assert {c.p for c in R.CASES} == {0.1, 0.5} and all(c.B == 2 and c.H == 2 for c in R.CASES)
    assert {c.N for c in R.CASES if c.family == "single"} == set(R.AE.SINGLE_PASS_NS)
    for dh in R.AE.STREAM_DH:
        ns = {c.N for c in R.CASES if c.family == "stream" and c.dh == dh}
        assert ns == ({257, 300} if dh == 64 else {1, 63, 64, 65, 129, 257}), (dh, ns)
    assert {R.AE.single_pass_nt(c.N) for c in R.CASES if c.family == "single"} == {2, 4, 6, 8, 10, 12, 13, 14, 16}
    assert len({c.seed for c in R.CASES}) == len(R.CASES) and all(c.seed >> 32 for c in R.CASES)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_kernel_rounding_stays_inside_half_the_bound_on_every_row(c):
    exact = R.check(c, R.restated(c))
    assert max(exact.values()) < 1e-6, exact                       # the restatement IS the definition when nothing is rounded
    ratios = R.check(c, R.restated(c, kernel_rounding=True), bound=R.KERNEL_ROUNDING_BOUND)
    print(R.case_id(c), "error / half bound", {k: f"{v:.3f}" for k, v in ratios.items()})
    assert max(ratios.values()) <= 1.0, (R.case_id(c), ratios)
    ref, got = R.reference(c), R.restated(c, kernel_rounding=True)
    none = ref["none"]
    assert bool((got["o"][none] == 0).all()) and bool((got["dq"][none] == 0).all())
    assert bool((ref["o"][none] == 0).all()) and bool((ref["dq"][none] == 0).all())


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_each_mistake_is_seen(mistake):
    over = [R.case_id(c) for c in R.CASES if max(R.check(c, R.restated(c, mistake)).values()) > 1.0]
    print(mistake, len(over), "cases over PER_ROW_BOUND")
    assert over, mistake
    # ... and exactly, by a probe, at a shape with more than one key tile
    c = next(k for k in R.CASES if k.family == "stream" and k.N == 129 and k.dh == 32)
    dec = R.probe_decode(c, lambda qkv, dout: R.restated_run(c, qkv, dout, mistake, kernel_rounding=True))
    m = R.case_mask(c)
    wrong = {n: int((dec[n] != m).sum()) for n in dec}
    print(mistake, "decisions a probe decodes differently", wrong)
    exact = {"mask_transposed": ("dv",), "head_index": ("fwd", "dv", "dq"), "tile_local_k": ("fwd", "dv", "dq"),
             "seed_low_only": ("fwd", "dv", "dq"), "bwd_unmasked": ("dq",)}
    for n in exact.get(mistake, ()):
        assert wrong[n] > 0, (mistake, n)
    if mistake in ("dv_unscaled", "rowsum_after_drop"):           # the mask is right, a value is not: the probe's values show it
        a = R.restated_run(c, *R.probe_inputs(c, "fwd_dv", 0), mistake, kernel_rounding=True)
        b = R.restated_run(c, *R.probe_inputs(c, "fwd_dv", 0), None, kernel_rounding=True)
        name = "dv" if mistake == "dv_unscaled" else "o"
        assert not torch.equal(a[name], b[name])


@pytest.mark.parametrize("c", PROBE_CASES, ids=R.case_id)
def test_probes_decode_the_mask_bit_for_bit(c):
    dec = R.probe_decode(c, lambda qkv, dout: R.restated_run(c, qkv, dout, None, kernel_rounding=True))
    m = R.case_mask(c)
    for n in ("fwd", "dv", "dq"):
        assert torch.equal(dec[n], m), (R.case_id(c), n, int((dec[n] != m).sum()))


def _within(count: np.ndarray, n: int, prob: float, what: str):
    sigma = math.sqrt(n * prob * (1.0 - prob))
    z = np.abs(np.asarray(count, dtype=np.float64) - n * prob) / sigma
    print(f"{what}: n = {n}, expected {prob:.5f}, worst {float(z.max()):.2f} sigma")
    assert float(z.max()) <= 5.0, (what, float(z.max()))


@pytest.mark.parametrize("p", (0.1, 0.5))
def test_mask_statistics(p):
    B, H, N = 4, 4, 256
    pe = R.p_eff(p)
    s0, s1 = R.BASE_SEED, R.BASE_SEED + 1
    m = R.keep_mask(s0, p, B, H, N).reshape(B * H, N, N)
    m1 = R.keep_mask(s1, p, B, H, N).reshape(B * H, N, N)
    mu = R.keep_mask(s0 ^ (1 << 40), p, B, H, N).reshape(B * H, N, N)            # differs in the upper word only
    _within(m.sum(), m.size, 1 - pe, "kept overall")
    _within(m.sum(axis=(1, 2)), N * N, 1 - pe, "kept per g")
    _within(m.sum(axis=(0, 2)), B * H * N, 1 - pe, "kept per query row")
    _within(m.sum(axis=(0, 1)), B * H * N, 1 - pe, "kept per key column")
    agree = (1 - pe) ** 2 + pe ** 2
    _within((m == m1).sum(), m.size, agree, "agreement of two seeds")
    _within((m == mu).sum(), m.size, agree, "agreement of two seeds that differ in the upper word")
    _within((m[:-1] == m[1:]).sum(), m[1:].size, agree, "agreement of g and g + 1")
    _within((m[:, :, :-1] == m[:, :, 1:]).sum(), m[:, :, 1:].size, agree, "agreement of (q, k) and (q, k + 1)")
    _within((m[:, :, 0::2] == m[:, :, 1::2]).sum(), m[:, :, 1::2].size, agree, "agreement of the two halves of a word")
    _within((m[:, :-1] == m[:, 1:]).sum(), m[:, 1:].size, agree, "agreement of (q, k) and (q + 1, k)")


def test_mask_is_a_function_of_seed_g_q_k_alone():
    seed, p = R.BASE_SEED + 3, 0.1
    small, big = R.keep_mask(seed, p, 2, 2, 17), R.keep_mask(seed, p, 2, 2, 40)
    assert np.array_equal(small, big[:, :, :17, :17])
    # g = b H + h: the same g under another (B, H) has the same mask
    assert np.array_equal(R.keep_mask(seed, p, 2, 3, 17).reshape(6, 17, 17), R.keep_mask(seed, p, 3, 2, 17).reshape(6, 17, 17))


def test_threshold_and_p_eff():
    top = 1.0 - 2.0 ** -16
    assert [R.threshold(p) for p in (0.0, 1e-6, 0.1, 0.5, top)] == [0, 0, 6554, 32768, 65535]
    assert R.p_eff(0.5) == 0.5 and R.p_eff(1e-6) == 0.0 and R.p_eff(top) == top and abs(R.p_eff(0.1) - 0.1) < 2.0 ** -17
    assert [R.threshold(p) for p in (-0.1, 1.0, 1.5, float("nan"), 0.999995)] == [-2] * 5
    assert not R.keep_mask(R.BASE_SEED, top, 1, 1, 64).all() and R.keep_mask(R.BASE_SEED, 0.0, 1, 1, 64).all()


@pytest.fixture(scope="module")
def lib():
    from noise_robust_vit_amd import _lib, build
    build.build()
    return _lib.load()


def test_library_threshold_is_the_restated_one(lib):
    for p in (0.0, 1e-6, 0.1, 0.25, 0.5, 0.9, 1.0 - 2.0 ** -16, -0.1, 1.0, 1.5, float("nan"), 0.999995, -0.0):
        assert lib.nrv_attn_drop_threshold(ctypes.c_float(p)) == R.threshold(p), p


def test_argument_errors_are_reported_before_any_launch(lib):
    f = ctypes.c_float
    sc = f(0.125)
    # nrv_attn_drop_fwd(qkv, out, lse, seed, p, B, N, H, dh, scale, stream)
    assert lib.nrv_attn_drop_fwd(None, 16, 16, 16, f(0.1), 1, 64, 1, 64, sc, None) == -1
    assert lib.nrv_attn_drop_fwd(16, 16, 16, None, f(0.1), 1, 64, 1, 64, sc, None) == -1                 # the seed pointer
    for bad in (-0.1, 1.0, float("nan"), 0.999995):
        assert lib.nrv_attn_drop_fwd(16, 16, 16, 16, f(bad), 1, 64, 1, 64, sc, None) == -2
    assert lib.nrv_attn_drop_fwd(16, 16, 16, 16, f(0.1), 1, 64, 1, 72, sc, None) == -2                   # head dim
    assert lib.nrv_attn_drop_fwd(16, 16, 16, 16, f(0.1), 1, 64, 1, 160, sc, None) == -2                  # wide heads: no dropout
    assert lib.nrv_attn_drop_fwd(16, 16, 16, 16, f(0.1), 0, 64, 1, 64, sc, None) == -2
    assert lib.nrv_attn_drop_fwd(1, 16, 16, 16, f(0.1), 1, 64, 1, 64, sc, None) == -5                    # qkv
    assert lib.nrv_attn_drop_fwd(16, 16, 16, 4, f(0.1), 1, 300, 1, 64, sc, None) == -5                   # seed: 8-byte aligned
    assert lib.nrv_attn_drop_fwd(16, 2, 16, 16, f(0.1), 1, 257, 16, 80, sc, None) == -5
    # nrv_attn_drop_bwd(qkv, out, dout, lse, dqkv, delta, seed, p, B, N, H, dh, scale, stream)
    for i in range(7):
        args = [16] * 7
        args[i] = None
        assert lib.nrv_attn_drop_bwd(*args, f(0.1), 1, 64, 1, 64, sc, None) == -1, i
    for bad in (-0.1, 1.0, float("nan")):
        assert lib.nrv_attn_drop_bwd(16, 16, 16, 16, 16, 16, 16, f(bad), 1, 64, 1, 64, sc, None) == -2
    assert lib.nrv_attn_drop_bwd(16, 16, 16, 16, 16, 16, 16, f(0.1), 1, 64, 1, 40, sc, None) == -2
    for i in (0, 1, 2, 4):
        args = [16] * 7
        args[i] = 8
        assert lib.nrv_attn_drop_bwd(*args, f(0.1), 1, 300, 2, 32, sc, None) == -5, i
    assert lib.nrv_attn_drop_bwd(16, 16, 16, 16, 16, 16, 12, f(0.1), 1, 64, 1, 64, sc, None) == -5
    # nrv_attn_drop_mask(seed, p, keep, B, H, N, stream)
    assert lib.nrv_attn_drop_mask(None, f(0.1), 16, 1, 1, 8, None) == -1
    assert lib.nrv_attn_drop_mask(16, f(0.1), None, 1, 1, 8, None) == -1
    assert lib.nrv_attn_drop_mask(16, f(1.0), 16, 1, 1, 8, None) == -2
    assert lib.nrv_attn_drop_mask(16, f(0.1), 16, 0, 1, 8, None) == -2
    assert lib.nrv_attn_drop_mask(16, f(0.1), 16, 1, 1, 0, None) == -2
    assert lib.nrv_attn_drop_mask(16, f(0.1), 16, 4096, 4096, 1 << 20, None) == -2                       # more blocks than a grid holds
    assert lib.nrv_attn_drop_mask(4, f(0.1), 16, 1, 1, 8, None) == -5


def test_header_binding_and_library_declare_the_entries_under_abi_19(lib):
    from noise_robust_vit_amd import _lib
    names = ["nrv_attn_drop_threshold", "nrv_attn_drop_fwd", "nrv_attn_drop_bwd", "nrv_attn_drop_mask"]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nrv.h")).read(), flags=re.S)
    assert re.search(r"#define\s+NRV_ABI_VERSION\s+19\b", text)
    assert _lib.ABI_VERSION == 19 and lib.nrv_abi_version() == 19
    for n in names:
        proto = re.search(r"\bint\s+" + n + r"\s*\(([^)]*)\)", text)
        assert proto, n
        assert n in _lib.SIGNATURES and len(_lib.SIGNATURES[n][1]) == len(proto.group(1).split(",")), n
        assert hasattr(lib, n)
    fwd = re.search(r"nrv_attn_drop_fwd\s*\(([^)]*)\)", text).group(1)
    assert "const uint64_t* seed_dev" in fwd and "float p" in fwd and "layout" not in fwd
