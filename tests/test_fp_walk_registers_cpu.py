"""The compiler's resource report of feat_prenet_walk_kernel<DROP> (csrc/decoder_step.hip), checked at build time: no GPU needed.

The walker runs 512 threads per workgroup = two waves per SIMD, so a lane has 256 registers, and it keeps 176 of them for weight fragments: the three
dropout forms compile to 252 / 255 / 254 VGPRs without scratch (profiles/fp_walk_registers.txt).  A compiler update or an edit that costs a few
registers turns into scratch traffic inside the tile loop, silently: the kernel stays bit-identical and only gets slow.  This test compiles the
translation unit with the library's flags and -Rpass-analysis=kernel-resource-usage and fails on any scratch, on more than 256 registers, or on
fewer than two waves per SIMD."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fcl-taco2_amd", "csrc")


def makefile_var(name):
    text = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^%s\s*\?=\s*(.*)$" % name, text, re.M).group(1).strip()


def test_walker_has_no_scratch_and_fits_two_waves_per_simd(tmp_path):
    hipcc = os.environ.get("HIPCC") or makefile_var("HIPCC")
    assert os.path.exists(hipcc), "%s is needed to build the library at all" % hipcc
    cmd = [hipcc, "--offload-arch=" + makefile_var("ARCH"), "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function"] + makefile_var("NOPK").split() + [
        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "decoder_step.hip"), "-o", str(tmp_path / "decoder_step.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    report, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+))", line)
        if not m:
            continue
        if m.group(1):
            name = m.group(1)
            report[name] = {}
        elif name:
            report[name][m.group(2).strip()] = int(m.group(3))
    walkers = {k: v for k, v in report.items() if "feat_prenet_walk_kernel" in k}
    assert len(walkers) == 3, sorted(report)  # the three dropout forms
    for k, v in walkers.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] + v["AGPRs"] <= 256, (k, v)
        assert v["Occupancy"] >= 2, (k, v)
