"""CPU test: the register budget of dist_kernel_v2_rank, from the compiler's own report and the code object metadata.

tests/test_abi.py guards dist_kernel_v2 by name; the nine instantiations that compare a rank-coded database
(PL in {12, 10, 8} x MODE_DIST, MODE_MASK, MODE_BGMM) sit at the same limit and carry, per block, the choice between
the full and the short instruction stream (tools/gen_block_asm.py).  One more live value across the compare loop
spills into it, which no functional test notices."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {0: "MODE_DIST", 3: "MODE_MASK", 5: "MODE_BGMM"}
KERNELS = ["_Z19dist_kernel_v2_rankILi%dELi%dEE" % (pl, mode) for pl in (12, 10, 8) for mode in MODES]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "poppunk_amd", "csrc", "ppk_dist.hip")
    asm = str(tmp_path_factory.mktemp("rank_budget") / "ppk_dist.s")
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
            assert vgprs <= 128, (name, vgprs)
            if "ELi0EE" in prefix:
                assert scratch == 0, (name, scratch)      # MODE_DIST: no scratch at all
            assert occupancy == 4 and lds == 81920, (name, occupancy, lds)
    assert seen == set(KERNELS)


def test_by_value_argument_at_offset_72(compiled):
    """the loop fetches the short flags, and the epilogue its parameters, through the kernarg segment pointer at the
    offset dist_kernel_v2 has them"""
    _, text = compiled
    meta = text[text.index("amdhsa.kernels:"):]
    n = 0
    for blk in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if name.startswith("_Z19dist_kernel_v2_rank"):
            n += 1
            byval = re.search(r"- \.offset:\s+(\d+)\n\s+\.size:\s+(\d+)\n\s+\.value_kind:\s+by_value", blk)
            assert byval and int(byval.group(1)) == 72, (name, byval and byval.group(0))
    assert n == 9


def test_no_scratch_in_the_compare_loops(compiled):
    """both loops of every instantiation (full / short block with the choice inside the statement, and the half block):
    nothing touches scratch between the loop header and the closing barrier; the full loop holds both streams"""
    _, text = compiled
    loops = 0
    for prefix in KERNELS:
        m = re.search(r"^(%s\w*):[^\n]*\n(.*?)^\.Lfunc_end" % prefix, text, re.S | re.M)
        assert m, prefix
        lines = m.group(2).split("\n")
        # a block's statement: its first ds_read is the stream's (the full block's follows the flag test and the branch)
        starts = [i for i, ln in enumerate(lines)
                  if "#ASMSTART" in ln and any("ds_read_b128 v[80:83]" in x for x in lines[i + 1:i + 4])]
        assert len(starts) == 2, "compare blocks not found in " + prefix
        # basic block -> the loop it belongs to, from the compiler's own annotations (as tests/test_abi.py does)
        owner, cur = [None] * len(lines), None
        for i, ln in enumerate(lines):
            lab = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)", ln)
            if lab:
                if "Loop Header" in ln:
                    cur = lab.group(1)
                else:
                    h = re.search(r"in Loop: Header=(BB\d+_\d+)", ln)
                    cur = h.group(1) if h else None
            owner[i] = cur
        selects = 0
        for b in starts:
            assert owner[b], (prefix, b)
            body = [ln for i, ln in enumerate(lines) if owner[i] == owner[b]]
            assert len(body) < 2500, (prefix, len(body))
            assert any("s_barrier" in ln for ln in body), prefix + ": the block's loop has no closing barrier"
            bad = [ln for ln in body if "scratch_" in ln]
            assert not bad, prefix + ": scratch access inside the compare loop: " + bad[0]
            selects += sum(1 for ln in body if re.match(r"\s*s_cbranch_scc1 \.Lppk_short_", ln))
            loops += 1
        assert selects == 1, prefix + ": one choice between the full and the short stream, in the full-block loop"
        # the counters stay pinned: no v_bcnt reads two VGPRs of the same bank
        bc = re.findall(r"v_bcnt_u32_b32 v(\d+), v(\d+), v(\d+)", m.group(2))
        assert len(bc) >= 80
        assert not [t for t in bc if int(t[1]) % 4 == int(t[2]) % 4], prefix + ": v_bcnt bank conflict"
    assert loops == 18
