"""The level-1 GEGLU projection pass (csrc/sta_ffgemm640.hip) is built to the last register of two waves per SIMD: sta.lib.build()
refuses a toolchain that spills it. The check on hand-written metadata, and on its translation unit (csrc/sta_ffgemm.hip, which
includes it) compiled here (hipcc cross-compiles without a GPU). Only register, scratch and LDS metadata are read."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd"))
from sta import isa_lint, lib  # noqa: E402

META = """\t.text
k:
\ts_endpgm
\t.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           40
        .value_kind:     by_value
    .group_segment_fixed_size: 0
    .name:           _ZN12_GLOBAL__N_126ff_geglu_c640_qfrag_kernelIDF16_EEvNS_2G6E
    .private_segment_fixed_size: %d
    .sgpr_count:     73
    .sgpr_spill_count: 0
    .vgpr_count:     256
    .vgpr_spill_count: %d
    .wavefront_size: 64
  - .agpr_count:     0
    .name:           other_kernel
    .private_segment_fixed_size: 64
    .vgpr_count:     12
    .vgpr_spill_count: 3
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
...
\t.end_amdgpu_metadata
"""


def test_kernel_metadata_and_the_no_spill_check():
    meta = lib.kernel_metadata(META % (0, 0))
    assert set(meta) == {"_ZN12_GLOBAL__N_126ff_geglu_c640_qfrag_kernelIDF16_EEvNS_2G6E", "other_kernel"}
    assert meta["other_kernel"] == {"private_segment_fixed_size": 64, "vgpr_count": 12, "vgpr_spill_count": 3}
    # only the kernels named for a source are held to it: the other kernel's scratch is its own business
    assert [n for n, _ in lib.check_no_spill("csrc/sta_ffgemm.hip", META % (0, 0))] == ["_ZN12_GLOBAL__N_126ff_geglu_c640_qfrag_kernelIDF16_EEvNS_2G6E"]
    assert lib.check_no_spill("csrc/sta_rowgemm.hip", META % (724, 188)) == []
    for scratch, spills in ((724, 188), (8, 0), (0, 1)):
        with pytest.raises(lib.StaLibraryError, match="spills"):
            lib.check_no_spill("csrc/sta_ffgemm.hip", META % (scratch, spills))
    with pytest.raises(lib.StaLibraryError, match="no kernel named"):
        lib.check_no_spill("csrc/sta_ffgemm.hip", "\t.text\n")


def test_c640_pass_compiles_without_spills_in_both_types():
    # built as part of the level-0 feed-forward's translation unit, with that unit's flags (tests/test_abi_dtype_cpu.py pins lib.SOURCES)
    host = lib.INCLUDED_SOURCES["sta_ffgemm640.hip"]
    assert host == "sta_ffgemm.hip" and "-ffinite-math-only" in lib.PER_SOURCE_FLAGS[host]
    src = os.path.join(lib.CSRC, host)
    assert src in lib.SOURCES and '#include "sta_ffgemm640.hip"' in open(src).read()
    text = open(isa_lint.compile_to_asm(src, lib.PER_SOURCE_FLAGS[host], [lib.INCLUDE, lib.CSRC])).read()
    found = dict(lib.check_no_spill(src, text))
    assert len(found) == 2 and any("IDF16_E" in n for n in found) and any("IDF16bE" in n for n in found), sorted(found)     # fp16, bf16
    for name, m in found.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)        # two waves per SIMD
        assert m["group_segment_fixed_size"] == 0       # the 90 KiB ring + bias table are dynamic LDS, sized at the launch
