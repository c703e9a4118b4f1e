"""Upsample.conv as four 2x2 sub-pixel convolutions of the half-resolution tensor (sta.fused.subpixel_weights, csrc/sta_conv.hip SUB):
the decomposition is exact, and the library exports its entry points."""
import pytest
import torch
import torch.nn.functional as F

# (B, Cin, Cout, output H, output W): the shapes of tests/test_conv_up2_subpixel_gpu.py
SHAPES = [(1, 64, 160, 64, 64), (2, 192, 320, 32, 32), (8, 128, 160, 16, 16), (3, 128, 320, 16, 16), (2, 64, 256, 64, 64), (3, 64, 160, 32, 32),
          (16, 64, 320, 64, 64)]


@pytest.mark.parametrize("B,Cin,Cout,H,W", SHAPES)
def test_subpixel_decomposition_is_exact(B, Cin, Cout, H, W):
    """conv2d(interpolate(x, 2, 'nearest'), w, padding=1) == the four 2x2 convolutions of the zero-padded x with the pre-summed taps, in
    float64 on unrounded sums: the two differ only by the summation order of exact products' roundings (1e-12)."""
    from sta import fused
    torch.manual_seed(Cin + Cout + H)
    x = torch.randn(B, Cin, H // 2, W // 2, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, dtype=torch.float64) / (9 * Cin) ** 0.5
    wsub = fused.subpixel_weights(w)
    assert wsub.shape == (4, Cout, Cin, 2, 2) and wsub.dtype == torch.float64
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, None, 1, 1)
    got = fused.subpixel_conv_reference(x, wsub)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-12


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_subpixel_weights_round_once(dtype):
    """16-bit weights: every tap is the fp32 sum (ky-major, kx-minor) of one, two or four weights, rounded once; the taps of a phase
    together hold each of the nine weights exactly once."""
    from sta import fused
    torch.manual_seed(1)
    w = (torch.randn(32, 64, 3, 3) / 24.0).to(dtype)
    ws = fused.subpixel_weights(w)
    assert ws.dtype == dtype
    f = w.float()
    assert torch.equal(ws[0, :, :, 0, 0], w[:, :, 0, 0]) and torch.equal(ws[3, :, :, 1, 1], w[:, :, 2, 2])
    assert torch.equal(ws[0, :, :, 1, 1], (((f[:, :, 1, 1] + f[:, :, 1, 2]) + f[:, :, 2, 1]) + f[:, :, 2, 2]).to(dtype))
    assert torch.equal(ws[3, :, :, 0, 0], (((f[:, :, 0, 0] + f[:, :, 0, 1]) + f[:, :, 1, 0]) + f[:, :, 1, 1]).to(dtype))
    assert torch.equal(ws[1, :, :, 1, 0], (f[:, :, 1, 0] + f[:, :, 1, 1] + f[:, :, 2, 0] + f[:, :, 2, 1]).to(dtype))
    assert torch.equal(ws[2, :, :, 0, 1], (f[:, :, 0, 1] + f[:, :, 0, 2] + f[:, :, 1, 1] + f[:, :, 1, 2]).to(dtype))
    total = fused.subpixel_weights(w.double()).sum(dim=(3, 4))
    assert (total - w.double().sum(dim=(2, 3))).abs().max().item() <= 1e-12


def test_library_exports_the_subpixel_entry_points():
    from sta import lib
    L = lib.load()
    for name in ("sta_conv3x3_up2_nhwc_supported", "sta_conv3x3_up2_stats_slots", "sta_conv3x3_up2_packed_w_bytes", "sta_conv3x3_up2_pack_w",
                 "sta_conv3x3_up2_nhwc"):
        assert name in lib.SYMBOLS and getattr(L, name) is not None
    # geometry of the H / 2 x W / 2 input: 32-multiple-wide, 16-wide, 8 x 8; a 16-wide, 8-high input has no tile and stays on the 3x3 path
    assert L.sta_conv3x3_up2_nhwc_supported(1, 64, 64, 64, 160) and L.sta_conv3x3_up2_nhwc_supported(2, 32, 32, 192, 320)
    assert L.sta_conv3x3_up2_nhwc_supported(3, 16, 16, 128, 320) and L.sta_conv3x3_up2_nhwc_supported(1, 512, 512, 256, 256)
    assert L.sta_conv3x3_nhwc_supported(1, 16, 32, 64, 160) and not L.sta_conv3x3_up2_nhwc_supported(1, 16, 32, 64, 160)
    assert not L.sta_conv3x3_up2_nhwc_supported(1, 63, 64, 64, 160) and not L.sta_conv3x3_up2_nhwc_supported(1, 64, 64, 32, 160)
    assert not L.sta_conv3x3_up2_nhwc_supported(1, 64, 64, 64, 96)
    assert L.sta_conv3x3_up2_packed_w_bytes(64, 160) == 160 * 64 * 16 * 2 and L.sta_conv3x3_up2_packed_w_bytes(32, 160) == 0
    assert L.sta_conv3x3_up2_stats_slots(64, 64) == 4 * L.sta_conv3x3_stats_slots(32, 32) == 64
    assert L.sta_conv3x3_up2_stats_slots(16, 16) == 8 and L.sta_conv3x3_up2_stats_slots(16, 32) == 0
    assert L.sta_conv3x3_up2_nhwc(0, 0, 0, 0, 0, 0, 0, 1, 64, 64, 64, 160, 1, 0) != 0 and "null pointer" in lib.last_error()
