"""MXFP8 (sta.mxfp8, csrc/sta_mxfp8.hip) without a GPU: the host restatement of the OCP MX quantiser that the GPU tests hold the
kernel to bit for bit (scale rule, saturation, zero / subnormal blocks, round-to-nearest-even ties), the hazard lint's view of the
block-scaled MFMA, and the --mxfp8 command-line refusals."""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd"))
from sta import isa_lint, mxfp8  # noqa: E402


def _scale_exp(block):
    amax = max(abs(float(v)) for v in block)
    if amax == 0:
        return 0
    return max(-127, min(127, math.floor(math.log2(amax)) - 8))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_reference_scale_rule_and_roundtrip(dtype):
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(7, 256, generator=g) * torch.logspace(-3, 3, 7).unsqueeze(1)).to(dtype)
    q, s = mxfp8.quant_rows_mx_reference(x)
    assert q.dtype == torch.float8_e4m3fn and q.shape == x.shape and s.dtype == torch.uint8 and s.shape == (7, 8)
    for r in range(7):
        for b in range(8):
            assert int(s[r, b]) == _scale_exp(x[r, 32 * b:32 * b + 32]) + 127
    back = mxfp8.dequant_mx(q, s)
    xf = x.float()
    X = torch.ldexp(torch.ones(7, 8), s.float() - 127).repeat_interleave(32, dim=1)
    sat = xf.abs() / X > 448
    # the e4m3 relative step is 2^-3 (half of it for rounding), its subnormal step 2^-9 X; quotients above 448 saturate
    assert ((back - xf).abs() <= 2.0 ** -4 * xf.abs() + 2.0 ** -10 * X)[~sat].all()
    assert torch.equal(back[sat], torch.sign(xf[sat]) * 448 * X[sat])
    assert q.float().abs().max() <= 448


def test_reference_saturates_zero_blocks_and_ties():
    x = torch.zeros(1, 128, dtype=torch.float32)
    # block 0: amax 510 -> X = 2^0, elements above 448 saturate
    x[0, 0], x[0, 1], x[0, 2], x[0, 3] = 510.0, -500.0, 448.0, 450.0
    # block 1 stays all zero
    # block 2: X = 2^0 (amax 256): ties between neighbouring e4m3 values round to the even code
    x[0, 64] = 256.0
    x[0, 65], x[0, 66], x[0, 67], x[0, 68] = 1.0625, 1.1875, -2.125, 2.375        # 1|1.125, 1.125|1.25, 2|2.25, 2.25|2.5
    x[0, 69] = 2.0 ** -10                                                          # half the smallest subnormal 2^-9: ties to 0
    x[0, 70] = 3 * 2.0 ** -10                                                      # 1.5 x 2^-9: ties to 2 x 2^-9
    # block 3: amax 3 * 2^-20 -> X = 2^-27; an element 2^-37 is half the smallest subnormal and ties to 0
    x[0, 96], x[0, 97] = 3 * 2.0 ** -20, 2.0 ** -37
    q, s = mxfp8.quant_rows_mx_reference(x.to(torch.bfloat16))
    v = q.float()[0]
    assert s.tolist() == [[127, 127, 127, 127 - 27]]
    assert v[:4].tolist() == [448.0, -448.0, 448.0, 448.0]
    assert (v[32:64] == 0).all() and (q.view(torch.uint8)[0, 32:64] == 0).all()
    assert v[65:71].tolist() == [1.0, 1.25, -2.0, 2.5, 0.0, 2 * 2.0 ** -9]
    assert v[96] == 3 * 2.0 ** 7 and v[97] == 0


def test_reference_subnormal_blocks():
    # fp16 subnormal block: amax 2^-20 -> X = 2^-28; bf16 values far below 2^-127 clamp the exponent to -127
    x16 = torch.full((1, 32), 2.0 ** -20, dtype=torch.float16)
    x16[0, 1] = 2.0 ** -24
    q, s = mxfp8.quant_rows_mx_reference(x16)
    assert int(s[0, 0]) == 127 - 28 and q.float()[0, 0] == 256.0 and q.float()[0, 1] == 16.0
    xb = torch.full((1, 32), 2.0 ** -130, dtype=torch.bfloat16)
    q, s = mxfp8.quant_rows_mx_reference(xb)
    assert int(s[0, 0]) == 0 and q.float()[0, 0] == 2.0 ** -3
    assert torch.equal(mxfp8.dequant_mx(q, s), xb.float())


def test_reference_matches_torch_cast_elementwise():
    """Per element the rule IS torch's e4m3fn cast of the clamped power-of-two quotient (round to nearest even)."""
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(64, 320, generator=g) * 5).half()
    q, s = mxfp8.quant_rows_mx_reference(x)
    X = torch.ldexp(torch.ones(64, 10), s.float() - 127).repeat_interleave(32, dim=1)
    assert torch.equal(q.view(torch.uint8), (x.float() / X).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))


def test_geglu_row_packing_is_a_documented_permutation():
    perm = mxfp8.pack_geglu_rows(128)
    assert sorted(perm.tolist()) == list(range(128))
    assert perm[:32].tolist() == list(range(32)) and perm[32:64].tolist() == list(range(64, 96))
    assert perm[64:96].tolist() == list(range(32, 64)) and perm[96:].tolist() == list(range(96, 128))
    w = torch.arange(128 * 4).view(128, 4)
    assert torch.equal(w[perm][torch.argsort(perm)], w)


def test_lint_knows_the_block_scaled_mfma():
    assert isa_lint._mfma_info("v_mfma_scale_f32_32x32x64_f8f6f4") == 16
    assert isa_lint._mfma_info("v_mfma_scale_f32_16x16x128_f8f6f4") == 8
    # the unscaled f8f6f4 rule is unchanged
    assert isa_lint._mfma_info("v_mfma_f32_32x32x64_f8f6f4") == 8
    assert isa_lint._mfma_info("v_mfma_f32_16x16x128_f8f6f4") == 8


def _kernel(*body):
    return "\t.text\nk_test:\n" + "\n".join("\t" + b for b in body) + "\n\ts_endpgm\n.Lfunc_end0:\n"


SCALED = "v_mfma_scale_f32_32x32x64_f8f6f4 v[0:15], v[16:23], v[24:31], v[0:15], v40, v41 op_sel_hi:[0,0,0]"


def test_lint_checks_scaled_mfma_results_and_scale_operands():
    read = "v_add_f32_e32 v50, v3, v3"
    # 16 passes: a vector read of D needs 16 + 4 wait states
    assert "mfma D -> read" in [f.rule for f in isa_lint.lint_text(_kernel(SCALED, "s_nop 15", "s_nop 2", read))]
    assert isa_lint.lint_text(_kernel(SCALED, "s_nop 15", "s_nop 3", read)) == []
    # the scale VGPRs are operands: a vector write right in front of the MFMA is a hazard
    assert "vector write -> mfma operand" in [f.rule for f in isa_lint.lint_text(_kernel("v_mov_b32_e32 v41, 0x7f", SCALED))]
    assert isa_lint.lint_text(_kernel("v_mov_b32_e32 v41, 0x7f", "s_nop 1", SCALED)) == []


def _parser():
    sys.path.insert(0, os.path.join(ROOT, "diffusion-spacetime-attn_amd", "scripts"))
    import _txt2img_common as c
    return c


def test_mxfp8_flag_needs_fixed_weights_and_excludes_fp8():
    c = _parser()
    p = c.build_parser("x.txt")
    ok = p.parse_args(["--plms", "--mxfp8", "--opt_epochs", "0"])
    assert ok.mxfp8 and not ok.fp8
    c.check_options(ok)
    with pytest.raises(SystemExit, match="--opt_epochs 0"):
        c.check_options(p.parse_args(["--plms", "--mxfp8"]))                 # default opt_epochs = 3
    with pytest.raises(SystemExit, match="exclusive"):
        c.check_options(p.parse_args(["--plms", "--mxfp8", "--fp8", "--opt_epochs", "0"]))
    c.check_options(p.parse_args(["--plms", "--fp8", "--opt_epochs", "0"]))  # --fp8 alone is unchanged
