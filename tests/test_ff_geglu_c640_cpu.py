"""The level-1 instance of the GEGLU projection pass (csrc/sta_ffgemm.hip, C = 640) is built to the last register of two waves per
SIMD: sta.lib.build() refuses a toolchain that spills it. The check on hand-written metadata, and on its translation unit
compiled here (hipcc cross-compiles without a GPU). Only register, scratch and LDS metadata are read."""
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
        .size:           48
        .value_kind:     by_value
    .group_segment_fixed_size: 0
    .name:           _ZN12_GLOBAL__N_121ff_geglu_qfrag_kernelIDF16_Li640EEEvNS_2FFE
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
    assert set(meta) == {"_ZN12_GLOBAL__N_121ff_geglu_qfrag_kernelIDF16_Li640EEEvNS_2FFE", "other_kernel"}
    assert meta["other_kernel"] == {"private_segment_fixed_size": 64, "vgpr_count": 12, "vgpr_spill_count": 3}
    # only the kernels named for a source are held to it: the other kernel's scratch is its own business
    assert [n for n, _ in lib.check_no_spill("csrc/sta_ffgemm.hip", META % (0, 0))] == ["_ZN12_GLOBAL__N_121ff_geglu_qfrag_kernelIDF16_Li640EEEvNS_2FFE"]
    assert lib.check_no_spill("csrc/sta_rowgemm.hip", META % (724, 188)) == []
    for scratch, spills in ((724, 188), (8, 0), (0, 1)):
        with pytest.raises(lib.StaLibraryError, match="spills"):
            lib.check_no_spill("csrc/sta_ffgemm.hip", META % (scratch, spills))
    with pytest.raises(lib.StaLibraryError, match="no kernel named"):
        lib.check_no_spill("csrc/sta_ffgemm.hip", "\t.text\n")


def test_c640_pass_compiles_without_spills_in_both_types():
    # one kernel template with the level-0 pass, in the feed-forward's translation unit and with that unit's flags
    host = "sta_ffgemm.hip"
    assert "-ffinite-math-only" in lib.PER_SOURCE_FLAGS[host]
    src = os.path.join(lib.CSRC, host)
    assert src in lib.SOURCES
    text = open(isa_lint.compile_to_asm(src, lib.PER_SOURCE_FLAGS[host], [lib.INCLUDE, lib.CSRC])).read()
    found = dict(lib.check_no_spill(src, text))
    assert len(found) == 4 and all("ff_geglu_qfrag_kernel" in n for n in found), sorted(found)
    for dt in ("IDF16_", "IDF16b"):                     # fp16, bf16
        for shape in ("Li320E", "Li640E"):              # level 0, level 1
            assert sum(dt in n and shape in n for n in found) == 1, (dt, shape, sorted(found))
    for name, m in found.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)        # two waves per SIMD
        assert m["group_segment_fixed_size"] == 0       # the 85 | 90 KiB ring + bias table are dynamic LDS, sized at the launch
