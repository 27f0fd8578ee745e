"""CPU checks of getFitnessScore's boundary (no GPU): both C-ABI symbols are declared, exported and bound; without a
device the engine cannot be created (NDT_ERR_NO_DEVICE) and the calls refuse bad arguments before touching one
(NDT_ERR_INVALID_ARG); the fitness kernels compile for gfx950 without scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = np.finfo(np.float64).max


def test_fitness_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    for name in ("ndt_fitness_score", "ndt_fitness_scores"):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in pkg.ABI_SYMBOLS
        assert getattr(L, name).argtypes is not None        # bound with a signature by lib()
    assert C.sizeof(pkg.Fitness) == 32
    for m in ("getFitnessScore", "fitness", "fitnessMany"):
        assert callable(getattr(pkg.NormalDistributionsTransform, m))


def test_no_device_and_invalid_arguments(pkg):
    L = pkg.lib()
    n, info = pkg.backend_info()
    if n <= 0:
        with pytest.raises(pkg.NdtError) as ei:
            pkg.NormalDistributionsTransform().getFitnessScore()
        assert ei.value.code == -2                           # NDT_ERR_NO_DEVICE: no CPU fallback
    T = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    f = pkg.Fitness()
    sq = (C.c_float * 4)()
    assert L.ndt_fitness_score(None, T, DBL_MAX, C.byref(f), None, 0) == -1
    assert L.ndt_fitness_score(None, None, DBL_MAX, C.byref(f), sq, 4) == -1
    assert L.ndt_fitness_scores(None, T, 1, DBL_MAX, C.byref(f)) == -1
    assert L.ndt_fitness_scores(None, T, 0, DBL_MAX, C.byref(f)) == -1
    assert L.ndt_fitness_scores(None, T, 1, DBL_MAX, None) == -1


def test_fitness_kernels_do_not_spill(tmp_path):
    src = os.path.join(ROOT, "slam-sam_amd", "csrc", "ndt_fitness.hip")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "f.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", ln)
        if m and name and "k_fit_" in name:
            usage.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    kernels = {re.search(r"k_fit_[a-z]+", k).group(0) for k in usage}
    assert kernels == {"k_fit_bounds", "k_fit_keys", "k_fit_gather", "k_fit_ends", "k_fit_query", "k_fit_shells",
                       "k_fit_reduce"}, kernels
    for k, u in usage.items():
        assert u["ScratchSize"] == 0, (k, u)
