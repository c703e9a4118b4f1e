"""The level-1 Linear + residual (+ LayerNorm) pass (csrc/sta_rows640.hip) is built close to the last register of two waves per
SIMD: sta.lib.build() refuses a toolchain that spills it. The kernel is listed, and its translation unit compiled here (hipcc
cross-compiles without a GPU) carries no spill. Only register, scratch and LDS metadata are read."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd"))
from sta import isa_lint, lib  # noqa: E402


def test_rows_c640_is_declared_and_listed():
    assert lib.INCLUDED_SOURCES["sta_rows640.hip"] == "sta_rowgemm.hip" and "-ffinite-math-only" in lib.PER_SOURCE_FLAGS["sta_rowgemm.hip"]
    assert os.path.exists(os.path.join(lib.CSRC, "sta_rows640.hip"))
    assert "rows640_kernel" in lib.NO_SPILL_KERNELS["sta_rows640.hip"]
    i, vp, l, f, sz = lib._i, lib._vp, lib._l, lib._f, lib._sz
    assert lib.SYMBOLS["sta_rows_c640_packed_w_bytes"] == (sz, [i, i])
    assert lib.SYMBOLS["sta_rows_c640_pack_w"] == (i, [vp, vp, i, i, i, vp])
    assert lib.SYMBOLS["sta_rows_c640"] == (i, [vp] * 8 + [l, i, i, f, i, i, i, vp])
    header = " ".join(open(os.path.join(lib.INCLUDE, "sta_xattn.h")).read().split())
    assert ("int sta_rows_c640(const void* a, const void* packed_w, const void* bias, const void* x, const void* gamma, const void* beta, "
            "void* s, void* y, long R, int C, int K, float eps, int y_qfrag, int max_workgroups, int dtype, void* stream);") in header


def test_rows_c640_compiles_without_spills_in_both_types():
    host = lib.INCLUDED_SOURCES["sta_rows640.hip"]
    src = os.path.join(lib.CSRC, host)
    assert src in lib.SOURCES
    text = open(isa_lint.compile_to_asm(src, lib.PER_SOURCE_FLAGS[host], [lib.INCLUDE, lib.CSRC])).read()
    assert lib.check_no_spill(src, text) == []          # the level-0 kernel of the unit is not held to it
    found = dict(lib.check_no_spill("sta_rows640.hip", text))
    assert len(found) == 4 and all("rows640_kernel" in n for n in found), sorted(found)
    for dt in ("IDF16_", "IDF16b"):                     # fp16, bf16
        for shape in ("Li640ELb1E", "Li2560ELb0E"):     # K = 640 with LayerNorm, K = 2560 without
            assert sum(dt in n and shape in n for n in found) == 1, (dt, shape, sorted(found))
    for name, m in found.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)        # two waves per SIMD
        assert m["group_segment_fixed_size"] == 0       # the 80 KiB ring, the tables and the exchange area are dynamic LDS
