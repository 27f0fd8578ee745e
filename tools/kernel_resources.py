"""VGPRs / SGPRs / scratch / LDS of the evaluators' kernels (hipcc cross-compiles; no GPU).
python tools/kernel_resources.py                    every k_derivatives instantiation, k_point_scores, k_d2d_eval, k_ct_eval,
                                                    k_vgicp_eval and the fixed-order row sum they share
python tools/kernel_resources.py FILE PATTERN ...   the kernels of csrc/FILE whose name matches PATTERN (extra hipcc arguments follow)"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam-sam_amd", "csrc")
# (a file that a tree does not have is skipped: the row sum was k_d2d_sum in ndt_d2d.hip before ndt_eval_rows.hip)
EVALUATORS = (("ndt_derivs.hip", "k_derivatives|k_point_scores"), ("ndt_d2d.hip", "k_d2d_eval|k_d2d_sum"), ("ndt_ct.hip", "k_ct_eval"),
              ("ndt_vgicp.hip", "k_vgicp_eval"),
              ("ndt_eval_rows.hip", "k_eval_rows_sum"))


def resources(file_name, pat, extra):
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                            "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, file_name), "-o", os.path.join(d, "d.o")] + extra,
                           capture_output=True, text=True)
        assert p.returncode == 0, p.stderr[-3000:]
    name, rows = None, {}
    for ln in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m: name = m.group(1)
        m = re.search(r"(VGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", ln)
        if m and name and re.search(pat, name): rows.setdefault(name, {})[m.group(1).split(" ")[0]] = int(m.group(2))
    return rows


def tag_of(nm):
    t = re.search(r"k_derivativesILb(\d)ELi(\d)ELi(\d)ELb(\d)", nm)
    if t: return "batch%s mode%s nb%s mbox%s" % t.groups()
    t = re.search(r"(k_point_scores)ILi(\d)E", nm)
    if t: return "%s<%s>" % t.groups()
    t = re.search(r"(k_d2d_eval|k_ct_eval|k_vgicp_eval)ILb(\d)ELb(\d)E", nm)
    if t: return "%s<hessian %s, d7 %s>" % t.groups()
    t = re.search(r"\d+(k_[a-z0-9_]+?)(?=[EIP])", nm)
    return t.group(1) if t else nm[:60]


jobs = [(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "k_derivatives")] if len(sys.argv) > 1 else \
       [(f, p) for f, p in EVALUATORS if os.path.exists(os.path.join(CSRC, f))]
for file_name, pat in jobs:
    for nm, u in resources(file_name, pat, sys.argv[3:]).items():
        print("%-32s VGPR %3d SGPR %3d scratch %3d occ %d LDS %d" % (tag_of(nm), u.get("VGPRs", -1), u.get("SGPRs", -1), u.get("ScratchSize", -1), u.get("Occupancy", -1), u.get("LDS", -1)))
