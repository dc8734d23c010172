"""CPU: the C-ABI library builds for gfx950, loads without a GPU, and exports exactly what include/nrv.h declares
(no compute calls here).  Also: argument errors are reported by return code before any launch."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib_path():
    from noise_robust_vit_amd import build
    return build.build()


def header_symbols():
    text = open(os.path.join(ROOT, "include", "nrv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nrv_[a-z0-9_]+)\s*\(", text)))


def test_header_binding_and_library_agree(lib_path):
    from noise_robust_vit_amd import _lib
    hdr = header_symbols()
    assert hdr == sorted(_lib.SIGNATURES), (set(hdr) ^ set(_lib.SIGNATURES))
    handle = ctypes.CDLL(lib_path)
    for name in hdr:
        assert hasattr(handle, name), f"{name} declared in nrv.h but not exported"
    assert handle.nrv_abi_version() == _lib.ABI_VERSION
    # and nothing else: every defined dynamic symbol of the library is declared in the header (no undeclared debug
    # entry points, no kernel variants reachable only through environment switches)
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[-1] for l in out.splitlines() if l.strip())
    host = [e for e in exported if not e.startswith("__hip_cuid_")]      # hipcc's per-translation-unit id objects
    assert host == hdr, (set(host) ^ set(hdr))


def test_product_has_no_environment_switches():
    """Nothing in the shipped package or its HIP sources reads the environment to pick a kernel variant."""
    pkg = os.path.join(ROOT, "noise_robust_vit_amd")
    hits = []
    for dp, _, fns in os.walk(pkg):
        if "_obj" in dp or "__pycache__" in dp:
            continue
        for fn in fns:
            if fn.endswith((".py", ".hip", ".hpp")):
                text = open(os.path.join(dp, fn)).read()
                if "getenv" in text or "os.environ" in text:
                    hits.append(fn)
    assert hits == [], hits


def test_product_sources_have_no_experiment_switches_and_empty_dev_hooks():
    """The HIP sources carry no preprocessor conditionals (no experiment / instrumentation variant can be switched on with a
    compiler flag); the only hook is <nrv_dev.hpp>, whose product version defines nothing but empty macros."""
    csrc = os.path.join(ROOT, "noise_robust_vit_amd", "csrc")
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith((".hip", ".hpp")):
            continue
        text = open(os.path.join(csrc, fn)).read()
        code = re.sub(r"//[^\n]*", "", text)
        assert not re.search(r"^\s*#\s*(ifdef|ifndef|if|elif|else)\b", code, flags=re.M), f"{fn}: conditional compilation"
        if fn != "nrv_dev.hpp":
            assert "s_memtime" not in code and "s_memrealtime" not in code, f"{fn}: clock read outside the dev hooks"
    hooks = open(os.path.join(csrc, "nrv_dev.hpp")).read()
    hooks = re.sub(r"//[^\n]*", "", hooks)
    for line in hooks.splitlines():
        line = line.strip()
        if not line or line == "#pragma once":
            continue
        m = re.match(r"#define\s+(NRV_[A-Z0-9_]+)(\([^)]*\))?\s*(.*)$", line)
        assert m, f"nrv_dev.hpp: unexpected line {line!r}"
        # empty, or the identity on its first argument (the tuning hooks NRV_TUNE_*)
        first = (m.group(2) or "()")[1:-1].split(",")[0].strip()
        assert m.group(3) in ("", f"({first})"), f"nrv_dev.hpp: hook {m.group(1)} is not empty: {m.group(3)!r}"


def test_product_device_code_reads_no_clock(lib_path, tmp_path):
    """Instrumented builds read s_memtime / s_memrealtime; the shipped device code must contain neither."""
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not available")
    import shutil
    so = shutil.copy(lib_path, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    cos = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert cos, "no gfx950 code objects found in the library"
    for f in cos:
        dis = subprocess.run([objdump, "-d", str(tmp_path / f)], capture_output=True, text=True, check=True).stdout
        assert "v_mfma" in dis or "buffer_" in dis or "global_" in dis      # really device code
        assert "s_memtime" not in dis and "s_memrealtime" not in dis, f


def test_loader_sets_prototypes_and_reports_errors(lib_path):
    from noise_robust_vit_amd import _lib
    lib = _lib.load()
    assert lib.nrv_error_string(0) == b"ok"
    # host-side argument validation happens before any launch: callable without a GPU
    assert lib.nrv_gemm_nt_bf16(None, 8, None, 8, None, 1, 8, 8, 8, 8, 0, None, None, 0, 0, 0, None, 0, 0, 0, 0, None) == -1
    # shapes are classified before anything else touches the (here: bogus, unaligned) pointers: the streaming kernels take
    # N > 256 and head dims 32 / 64 / 80 / 96 / 128 (the call then fails on the alignment check, -5), other dims are refused
    assert lib.nrv_attn_fwd(1, 1, 1, 1, 300, 1, 64, ctypes.c_float(0.125), 0, None) == -5       # N > 256: accepted shape
    assert lib.nrv_attn_fwd(1, 1, 1, 1, 257, 16, 80, ctypes.c_float(0.125), 0, None) == -5      # vit_h_14 geometry
    assert lib.nrv_attn_fwd(1, 1, 1, 1, 10, 1, 72, ctypes.c_float(0.125), 0, None) == -2        # unsupported head dim
    assert lib.nrv_attn_fwd(1, 1, 1, 1, 197, 12, 64, ctypes.c_float(0.125), 3, None) == -5      # blocked layouts: single-pass shapes
    assert lib.nrv_attn_fwd(1, 1, 1, 1, 300, 1, 64, ctypes.c_float(0.125), 1, None) == -2       # ... not the streaming kernels
    assert lib.nrv_attn_fwd(1, 1, 1, 1, 197, 12, 64, ctypes.c_float(0.125), 4, None) == -2      # unknown layout bit
    assert lib.nrv_gather_rows_f32(16, 16, 16, 4, 0, 64, None) == -2                            # ABI 11: the source-row count is required
    assert lib.nrv_bgemm(None, 1, 1, 1, 0, 0, 16, 1, 1, 1, 0, 0, 16, 0, 1, 1, 0, 0, 1, 1, 8, 8, 8, ctypes.c_float(1.0), None) == -1
    assert lib.nrv_attn_sinkhorn_fwd(1, 1, 1, 1, 1, 300, 1, 64, ctypes.c_float(0.125), None) == -2   # Sinkhorn: N <= 256 only
    for bad in (0.0, -0.125, float("nan")):          # ... and scale > 0 only: the forward scales the maximum of the raw scores
        assert lib.nrv_attn_sinkhorn_fwd(1, 1, 1, 1, 1, 197, 1, 64, ctypes.c_float(bad), None) == -2
        assert lib.nrv_attn_sinkhorn_bwd(1, 1, 1, 1, 1, 1, 197, 1, 64, ctypes.c_float(bad), None) == -2
    assert lib.nrv_attn_sinkhorn_fwd(1, 1, 1, 1, 1, 197, 1, 64, ctypes.c_float(0.125), None) == -5   # a good scale: on to the alignment check
    assert lib.nrv_layernorm_fwd(16, 0, 16, 16, 16, 16, 16, 4, 12, ctypes.c_float(1e-5), None) == -2   # dim % 8
    assert b"shape" in lib.nrv_error_string(-2)
    with pytest.raises(_lib.NrvError):
        _lib.check(-4, "demo")
    assert lib.nrv_gemm_tn_workspace(3072, 768, 50432) == 7 * 3072 * 768 * 4 + 7 * 3072 * 4     # 36 tiles -> 7 splits (+ bias slabs)
    assert lib.nrv_layernorm_bwd_workspace(50432, 768) == 1024 * 2 * 768 * 4


def test_missing_library_is_loud(monkeypatch, tmp_path):
    from noise_robust_vit_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(_lib.NrvError, match="no fallback"):
        _lib.load()
