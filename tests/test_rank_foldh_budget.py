"""CPU test: the register budget of dist_kernel_v2_foldh (the kernel of the holder pair, in the three modes the rank
kernel has), from the compiler's report and the code object's metadata as tests/test_rank_fold2_budget.py reads them: at
most 128 VGPRs, no scratch, at most 81 920 B of LDS, occupancy 4; DistParams at kernarg offset 72; the entries are added
with 64-bit LDS atomics."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["_Z20dist_kernel_v2_foldhILi%dEE" % mode for mode in (0, 3, 5)]      # MODE_DIST, MODE_MASK, MODE_BGMM


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "poppunk_amd", "csrc", "ppk_dist.hip")
    asm = str(tmp_path_factory.mktemp("foldh_budget") / "ppk_dist.s")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "--cuda-device-only", "-S", "-o", asm, src,
                          "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, cwd=os.path.dirname(src), timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stderr, open(asm).read()


def test_registers_scratch_occupancy_and_lds(compiled):
    remarks, _ = compiled
    seen = set()
    for b in re.split(r"remark: Function Name: ", remarks)[1:]:
        name = b.split()[0]
        for prefix in KERNELS:
            if not name.startswith(prefix):
                continue
            seen.add(prefix)
            vgprs = int(re.search(r" VGPRs: (\d+)", b).group(1))
            scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
            occupancy = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
            lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
            assert vgprs <= 128 and scratch == 0 and lds <= 81920 and occupancy == 4, (name, vgprs, scratch, lds, occupancy)
    assert seen == set(KERNELS)


def test_metadata_and_the_correction_block(compiled):
    _, text = compiled
    meta = text[text.index("amdhsa.kernels:"):]
    n = 0
    for blk in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if name.startswith("_Z20dist_kernel_v2_foldh"):
            n += 1
            byval = re.search(r"- \.offset:\s+(\d+)\n\s+\.size:\s+(\d+)\n\s+\.value_kind:\s+by_value", blk)
            assert byval and int(byval.group(1)) == 72, (name, byval and byval.group(0))
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
            assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) <= 81920, name
            assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 128, name
    assert n == 3
    for prefix in KERNELS:
        m = re.search(r"^(%s\w*):[^\n]*\n(.*?)^\.Lfunc_end" % prefix, text, re.S | re.M)
        assert m, prefix
        assert "ds_add_u64" in m.group(2), prefix + ": the entries are added with 64-bit LDS atomics"
        assert "scratch_" not in m.group(2), prefix
