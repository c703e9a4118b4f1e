"""The SpatialTransformer tail as one pass (csrc/sta_rowstail.hip, sta.fused.ff_tail*): the identity behind it in float64, the
bindings and the header, and both instantiations compiled here inside sta_ffgemm.hip's translation unit (hipcc cross-compiles
without a GPU) without a spill at two waves per SIMD. Only register, scratch and LDS metadata of the assembly are read."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd"))
from sta import fused, isa_lint, lib  # noqa: E402


@pytest.mark.parametrize("conv", [True, False])
@pytest.mark.parametrize("b2,bp", [(True, True), (True, False), (False, True), (False, False)])
def test_ff_tail_weights_single_gemm_equals_the_two_stages_in_float64(conv, b2, bp):
    """out = x_in + [h | x2] [W' | Wp]^T + b' with (W', b') = ff_tail_weights against x3 = x2 + net2(h), out = x_in + proj_out(x3),
    all in float64 on random weights: equal to 1e-12 relative (of the largest |out|). Without any bias b' is None."""
    C, inner, R = 48, 192, 40
    g = torch.Generator().manual_seed(3 + 2 * b2 + bp)
    net2 = torch.nn.Linear(inner, C, bias=b2).double()
    proj = (torch.nn.Conv2d(C, C, 1, bias=bp) if conv else torch.nn.Linear(C, C, bias=bp)).double()
    with torch.no_grad():
        for p in list(net2.parameters()) + list(proj.parameters()):
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64))
    h, x2, x_in = (torch.randn(R, n, generator=g, dtype=torch.float64) for n in (inner, C, C))
    w, b = fused.ff_tail_weights(net2, proj)
    assert w.dtype == torch.float64 and w.shape == (C, inner) and ((b is None) == (not b2 and not bp))
    wp = proj.weight.detach().reshape(C, C)
    one = x_in + torch.cat([h, x2], dim=1) @ torch.cat([w, wp], dim=1).t() + (0.0 if b is None else b)
    with torch.no_grad():
        x3 = x2 + net2(h)
        two = x_in + (proj(x3.t().reshape(1, C, R, 1)).reshape(C, R).t() if conv else proj(x3))
    assert (one - two).abs().max() <= 1e-12 * two.abs().max()


def test_ff_tail_weights_rounds_16_bit_products_once():
    """16-bit weights: the products are taken in fp32 and W' is rounded once to the weights' dtype; b' stays fp32."""
    g = torch.Generator().manual_seed(9)
    net2, proj = torch.nn.Linear(64, 16).half(), torch.nn.Conv2d(16, 16, 1).half()
    with torch.no_grad():
        for p in list(net2.parameters()) + list(proj.parameters()):
            p.copy_(torch.randn(p.shape, generator=g).half())
    w, b = fused.ff_tail_weights(net2, proj)
    wp = proj.weight.detach().reshape(16, 16).double()
    assert w.dtype == torch.float16 and b.dtype == torch.float32
    exact = wp @ net2.weight.detach().double()
    assert ((w.double() - exact).abs() <= 2.0 ** -11 * exact.abs() * (1 + 1e-3) + 1e-7).all()
    assert torch.allclose(b.double(), wp @ net2.bias.detach().double() + proj.bias.detach().double(), rtol=1e-5, atol=1e-5)


def test_ff_tail_is_declared_and_listed():
    # built at the end of the feed-forward passes' translation unit (the set of units is pinned by tests/test_abi_dtype_cpu.py)
    assert lib.INCLUDED_SOURCES["sta_rowstail.hip"] == "sta_ffgemm.hip" and "-ffinite-math-only" in lib.PER_SOURCE_FLAGS["sta_ffgemm.hip"]
    assert os.path.exists(os.path.join(lib.CSRC, "sta_rowstail.hip"))
    assert '#include "sta_rowstail.hip"' in open(os.path.join(lib.CSRC, "sta_ffgemm.hip")).read()
    assert "rows_tail_kernel" in lib.NO_SPILL_KERNELS["sta_rowstail.hip"]
    i, vp, l, sz = lib._i, lib._vp, lib._l, lib._sz
    assert lib.SYMBOLS["sta_ff_tail_packed_w_bytes"] == (sz, [i, i])
    assert lib.SYMBOLS["sta_ff_tail_pack_w"] == (i, [vp, vp, i, i, i, vp])
    assert lib.SYMBOLS["sta_ff_tail"] == (i, [vp] * 7 + [l, l, i, i, i, i, vp])
    header = " ".join(open(os.path.join(lib.INCLUDE, "sta_xattn.h")).read().split())
    assert "size_t sta_ff_tail_packed_w_bytes(int C, int inner);" in header
    assert "int sta_ff_tail_pack_w(const void* wcat, void* packed, int C, int inner, int dtype, void* stream);" in header
    assert ("int sta_ff_tail(const void* h, const void* x2, const void* packed_w, const float* bias, const void* x_in, void* out, float* stats, "
            "long rows_per_image, long R, int C, int inner, int max_workgroups, int dtype, void* stream);") in header
    assert fused.FF_TAIL_PROJ_OUT_C320 is True and fused.FF_TAIL_PROJ_OUT_C640 is True and fused.FF_TAIL_PASS_ROWS == {320: 256, 640: 128}


def test_ff_tail_compiles_without_spills_in_both_types():
    host = lib.INCLUDED_SOURCES["sta_rowstail.hip"]
    src = os.path.join(lib.CSRC, host)
    assert src in lib.SOURCES
    text = open(isa_lint.compile_to_asm(src, lib.PER_SOURCE_FLAGS[host], [lib.INCLUDE, lib.CSRC])).read()
    lib.check_no_spill(src, text)                       # the unit's own pinned kernels still hold
    found = dict(lib.check_no_spill("sta_rowstail.hip", text))
    assert len(found) == 4 and all("rows_tail_kernel" in n for n in found), sorted(found)
    for dt in ("IDF16_", "IDF16b"):                     # fp16, bf16
        for shape in ("Li320E", "Li640E"):
            assert sum(dt in n and shape in n for n in found) == 1, (dt, shape, sorted(found))
    for name, m in found.items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)        # two waves per SIMD
        assert m["group_segment_fixed_size"] == 0       # ring and table are dynamic LDS
    fixed, padded = isa_lint.fix_text(text)
    assert padded == [] and isa_lint.lint_text(fixed) == []          # nothing in the unit needs the hazard lint's padding
