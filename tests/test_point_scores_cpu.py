"""CPU checks of the per-point scoring boundary (no GPU): the new C-ABI symbols are declared, exported and bound; without
a device the engine cannot be created (NDT_ERR_NO_DEVICE) and the calls refuse bad arguments before touching one
(NDT_ERR_INVALID_ARG); the Python mirror validates its arguments; k_point_scores and the compaction kernels compile for
gfx950 without scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ndt_score_points", "ndt_score_points_device", "ndt_filter_source_device", "ndt_filter_source", "ndt_source_size")


def test_symbols_declared_exported_and_bound(pkg):
    hdr = open(os.path.join(ROOT, "include", "ndt_hip.h")).read()
    L = pkg.lib()
    for name in NEW:
        assert re.search(r"\b(int|int64_t) %s\s*\(" % name, hdr), name
        assert name in pkg.ABI_SYMBOLS
        assert getattr(L, name).argtypes is not None        # bound with a signature by lib()
    assert re.search(r"#define NDT_HIP_ABI_VERSION 3\b", hdr) and L.ndt_abi_version() == 3
    for m in ("scorePoints", "scorePointsDevice", "filterSource", "filterSourceDevice", "sourceSize"):
        assert callable(getattr(pkg.NormalDistributionsTransform, m))
    adapter = open(os.path.join(ROOT, "include", "ndt_hip", "ndt_hip.hpp")).read()
    for m in ("scorePoints", "nearestVoxelScoreEachPoint", "calculateNearestVoxelScoreEachPoint", "filterSource"):
        assert re.search(r"\b%s\s*\(" % m, adapter), m


def test_no_device_and_invalid_arguments(pkg):
    L = pkg.lib()
    n, info = pkg.backend_info()
    if n <= 0:
        with pytest.raises(pkg.NdtError) as ei:
            pkg.NormalDistributionsTransform().scorePoints(np.eye(4))
        assert ei.value.code == -2                           # NDT_ERR_NO_DEVICE: no CPU fallback
    T = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    d = (C.c_double * 4)()
    f = (C.c_float * 12)()
    m = C.c_size_t(7)
    assert L.ndt_score_points(None, T, d, None, None, None, 4) == -1
    assert L.ndt_score_points(None, None, None, None, None, None, 0) == -1
    assert L.ndt_score_points_device(None, T, None, None, None, None, 0) == -1
    assert L.ndt_filter_source(None, T, 0.5, 0, f, None, 4, C.byref(m)) == -1
    assert L.ndt_filter_source_device(None, T, 0.5, 0, None, None, None, None, 0, C.byref(m)) == -1
    assert L.ndt_source_size(None) == -1
    assert m.value == 7                                      # nothing was written


class _NoEngine:
    """The mirror's argument checks run before the C call: a stand-in handle is enough."""

    def __init__(self, pkg):
        self.obj = pkg.NormalDistributionsTransform.__new__(pkg.NormalDistributionsTransform)
        self.obj._h = C.c_void_p()


def test_python_mirror_validates_its_arguments(pkg):
    ndt = _NoEngine(pkg).obj
    with pytest.raises(ValueError):
        ndt.scorePoints(np.eye(4), fields=["score", "nope"])
    bad = np.eye(4)
    bad[1, 3] = np.nan
    for call in (lambda: ndt.scorePoints(bad), lambda: ndt.filterSource(bad, 0.5),
                 lambda: ndt.filterSourceDevice(bad, 0.5, False, 0, 0, 0, None, 0),
                 lambda: ndt.scorePointsDevice(bad, None, None, None, None, 0),
                 lambda: ndt.scorePoints(np.eye(3))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(pkg.NdtError) as ei:                  # a NULL handle reaches the C call and is refused there
        ndt.sourceSize()
    assert ei.value.code == -1
    names = [f for f, _ in pkg.NormalDistributionsTransform.POINT_SCORE_FIELDS]
    assert names == ["score", "nearest_voxel_score", "n_neighbors", "best_voxel"]


def resource_usage(src, pattern, tmp_path):
    """Per kernel whose name contains `pattern`: the figures the compiler's kernel-resource-usage remarks give for the
    gfx950 code object, as tools/kernel_resources.py reads them."""
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "slam-sam_amd", "csrc", src),
                        "-o", str(tmp_path / "k.o")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", ln)
        if m and name and pattern in name:
            usage.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    return usage


def test_point_score_kernel_does_not_spill(tmp_path):
    usage = resource_usage("ndt_derivs.hip", "k_point_scores", tmp_path)
    nbs = sorted(int(re.search(r"k_point_scoresILi(\d)E", k).group(1)) for k in usage)
    assert nbs == [0, 1, 2, 3, 4, 5, 6], nbs               # every neighbourhood, both record formats
    for k, u in usage.items():
        assert u["ScratchSize"] == 0, (k, u)


def test_compaction_kernels_do_not_spill(tmp_path):
    usage = resource_usage("ndt_point_scores.hip", "k_filter_", tmp_path)
    kernels = {re.search(r"k_filter_[a-z]+", k).group(0) for k in usage}
    assert kernels == {"k_filter_count", "k_filter_scan", "k_filter_emit"}, kernels
    for k, u in usage.items():
        assert u["ScratchSize"] == 0, (k, u)


def test_the_compaction_has_one_definition():
    """The ballot, the block count and the emit position are defined in ndt_compact_device.h and nowhere else, the
    filter's, the deskew's and the unprojection's kernels call them, and the block counts have ONE scan kernel."""
    csrc = os.path.join(ROOT, "slam-sam_amd", "csrc")
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip", ".cpp"))}
    for fn in ("compact_ballot", "compact_block_count", "compact_position"):
        defs = [f for f, text in sources.items() if re.search(r"\b(unsigned long long|void|unsigned int) %s\(" % fn, text)]
        assert defs == ["ndt_compact_device.h"], (fn, defs)
        for f in ("ndt_point_scores.hip", "ndt_deskew.hip", "ndt_unproject.hip"):
            assert re.search(r"\b%s\(" % fn, sources[f]), (fn, f)
    # nobody else writes the arithmetic out: a ballot's popcount into a per-wave word, the lanes below in a ballot
    for f, text in sources.items():
        if f != "ndt_compact_device.h" and f.startswith(("ndt_point_scores", "ndt_deskew", "ndt_unproject")):
            assert "__ballot" not in text and "__popcll" not in text, f
    scans = [(f, m.group(1)) for f, text in sources.items()
             for m in re.finditer(r"__global__[^{;]*?\b(k_\w*scan)\(([^)]*)\)", text)
             if re.search(r"\bcounts\b.*\bnb\b.*\btotal\b", m.group(2), re.S)]
    assert scans == [("ndt_point_scores.hip", "k_filter_scan")], scans
