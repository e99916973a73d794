"""The lane-per-HSP rows kernel of the gapped stage keeps nothing in scratch memory.

`k_gapped_rows<160,4,18>` and `<192,4,18>` run 4 wavefronts on each of the chip's 1 024 SIMDs.  With 120 bytes of scratch
per lane the live scratch was 31 MB, as much as all L2 together, and its traffic pushed the database words and the HSP
records out of L2.  The kernel source is written so that no vector register has to be spilled at
128 registers; this test compiles it and reads the resource figures from the code object's metadata, so that an edit
which brings spills back fails here instead of costing milliseconds unseen.

No GPU is needed: the source is compiled for gfx950, device side only, with the flags of the library build.
"""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pangea-plus_amd")


def _hipcc():
    p = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return p if os.path.exists(p) else None


pytestmark = pytest.mark.skipif(_hipcc() is None, reason="hipcc is not installed")

# (MAXL, WAVES, D) -> limits.  Scratch, vector registers and LDS as this kernel's own compile gives them:
#                                  scratch  VGPRs  LDS        (parent commit: scratch 120, VGPRs 128, LDS as here)
LIMITS = {
    (160, 4, 18): dict(scratch=0, vgpr=128, lds=9728),   # this build: scratch 0, VGPRs 127, LDS  9 728
    (192, 4, 18): dict(scratch=0, vgpr=128, lds=10752),  # this build: scratch 0, VGPRs 127, LDS 10 752
}

# Every instantiation that runs `gap_round` (the rows of both cell formats come from one function, greedy_rows_lean, so an
# edit for one format can move the other's registers): the figures of the compile before the two row functions became one.
# The wavefronts per SIMD follow from the registers (512 / VGPRs, the launch asks for WAVES), the wavefronts per CU from the LDS.
#                            VGPRs  scratch  spilled VGPRs  LDS
ROWS_FIGURES = {
    (160, 4, 18): dict(vgpr=127, scratch=0, vgpr_spills=0, lds=9728),
    (192, 4, 18): dict(vgpr=127, scratch=0, vgpr_spills=0, lds=10752),
    (320, 3, 18): dict(vgpr=155, scratch=0, vgpr_spills=0, lds=14848),
    (512, 2, 18): dict(vgpr=155, scratch=0, vgpr_spills=0, lds=20992),
    (512, 2, 40): dict(vgpr=256, scratch=32, vgpr_spills=12, lds=21504),
}
# (FLAT, MAXL, WAVES)
POOL_FIGURES = {
    (0, 160, 4): dict(vgpr=128, scratch=68, vgpr_spills=26, lds=9728),
    (1, 160, 4): dict(vgpr=128, scratch=64, vgpr_spills=25, lds=9728),
    (0, 192, 4): dict(vgpr=128, scratch=68, vgpr_spills=26, lds=10752),
    (1, 192, 4): dict(vgpr=128, scratch=64, vgpr_spills=25, lds=10752),
    (0, 320, 3): dict(vgpr=167, scratch=0, vgpr_spills=0, lds=14848),
    (1, 320, 3): dict(vgpr=167, scratch=0, vgpr_spills=0, lds=14848),
    (0, 512, 2): dict(vgpr=175, scratch=0, vgpr_spills=0, lds=20992),
    (1, 512, 2): dict(vgpr=173, scratch=0, vgpr_spills=0, lds=20992),
}


def _base_flags():
    spec = importlib.util.spec_from_file_location("_pgx_build_flags", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.BASE_FLAGS)  # (not FLAGS: a measurement build's -D switches are not the shipped kernel)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gapped_asm") / "gapped.s")
    cmd = [_hipcc()] + _base_flags() + ["-x", "hip", "--cuda-device-only", "-S", os.path.join(PKG, "csrc", "gapped.hip"), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    found = {}  # rows: (MAXL, WAVES, D); pool: ("pool", FLAT, MAXL, WAVES)
    for blk in meta.split("  - .agpr_count")[1:]:
        def field(key):
            return re.search(r"\.%s:\s+(\S+)" % key, blk).group(1)
        m = re.match(r"_ZN3pgx13k_gapped_rowsILi(\d+)ELi(\d+)ELi(\d+)EEE", field("name"))
        mp = re.match(r"_ZN3pgx13k_gapped_poolILb([01])ELi(\d+)ELi(\d+)EEE", field("name"))
        if m or mp:
            inst = tuple(int(x) for x in m.groups()) if m else ("pool",) + tuple(int(x) for x in mp.groups())
            found[inst] = dict(
                scratch=int(field("private_segment_fixed_size")), vgpr=int(field("vgpr_count")),
                lds=int(field("group_segment_fixed_size")), vgpr_spills=int(field("vgpr_spill_count")))
    return found


@pytest.mark.parametrize("inst", sorted(LIMITS))
def test_rows_kernel_has_no_scratch(kernels, inst):
    assert inst in kernels, "k_gapped_rows<%d,%d,%d> is not in the code object: %s" % (inst + (sorted(map(str, kernels)),))
    got, lim = kernels[inst], LIMITS[inst]
    print("k_gapped_rows<%d,%d,%d>:" % inst, got)
    assert got["scratch"] <= lim["scratch"], got
    assert got["vgpr_spills"] == 0, got
    # 4 wavefronts per SIMD: at most 128 registers (the count covers vector and accumulation registers)
    assert got["vgpr"] <= lim["vgpr"], got
    # 16 wavefronts per CU share its LDS: no more than before
    assert got["lds"] <= lim["lds"], got


def _held(name, got, lim):
    print(name, got)
    for key in ("vgpr", "scratch", "vgpr_spills", "lds"):
        assert got[key] <= lim[key], (name, key, got, lim)


@pytest.mark.parametrize("inst", sorted(ROWS_FIGURES))
def test_rows_kernel_keeps_its_figures(kernels, inst):
    assert inst in kernels, "k_gapped_rows<%d,%d,%d> is not in the code object: %s" % (inst + (sorted(map(str, kernels)),))
    _held("k_gapped_rows<%d,%d,%d>:" % inst, kernels[inst], ROWS_FIGURES[inst])


@pytest.mark.parametrize("inst", sorted(POOL_FIGURES))
def test_pool_kernel_keeps_its_figures(kernels, inst):
    assert ("pool",) + inst in kernels, "k_gapped_pool<%d,%d,%d> is not in the code object: %s" % (inst + (sorted(map(str, kernels)),))
    _held("k_gapped_pool<%d,%d,%d>:" % inst, kernels[("pool",) + inst], POOL_FIGURES[inst])
