"""The Upsample 3x3 convolutions as four 2x2 sub-pixel passes (csrc/sta_conv.hip SUB, sta_conv3x3_up2_nhwc) on the GPU: the kernel against
its own arithmetic, the pack against its documented layout, the result against the operation it replaces, the statistics epilogue,
and the host routing (switch, repack, support query)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

# (B, Cin, Cout, output H, output W)
CASES = [
    (1, 64, 160, 64, 64),      # GEO 0, four low-res tiles: every border
    (2, 192, 320, 32, 32),     # GEO 1, two parts, six channel steps
    (8, 128, 160, 16, 16),     # GEO 2
    (3, 128, 320, 16, 16),     # GEO 2, odd batch: the last tile holds one image
    (2, 64, 256, 64, 64),      # NTW = 4
    (3, 64, 160, 32, 32),      # tile count not a multiple of 8: plain item order
    (16, 64, 320, 64, 64),     # 512 items: the persistent loop crosses tiles and phases
]


@pytest.fixture(autouse=True)
def _kernels_at_every_size(monkeypatch):
    """The product routes launches with few work items to the library (sta.fused.CONV_MIN_ITEMS); these tests cover small shapes too."""
    from sta import fused
    monkeypatch.setattr(fused, "CONV_MIN_ITEMS", 1)


@functools.lru_cache(maxsize=None)
def _case(B, Cin, Cout, H, W, dtype):
    """Operands and references of a case, computed once: x, w, bias, res (16 bit, CPU), wsub = subpixel_weights(w) as rounded,
    ref2 = the float64 2x2 convolutions of the same 16-bit operands, ref3 = the fp32 3x3 convolution of the upsampled input,
    S = sum |W'_16| |x| (the first-order bound on rounding every summed weight once, in units of EPS)."""
    from sta import fused
    g = torch.Generator().manual_seed(Cin + Cout + H)
    x = torch.randn(B, Cin, H // 2, W // 2, generator=g).to(dtype)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).to(dtype)
    bias = (0.5 * torch.randn(Cout, generator=g)).to(dtype)
    res = torch.randn(B, Cout, H, W, generator=g).to(dtype)
    wsub = fused.subpixel_weights(w)
    ref2 = fused.subpixel_conv_reference(x.double(), wsub.double())
    ref3 = F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w.float(), None, 1, 1)
    S = fused.subpixel_conv_reference(x.double().abs(), wsub.double().abs())
    return x, w, bias, res, wsub, ref2, ref3, S


def _nhwc(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("B,Cin,Cout,H,W", CASES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("epi", [False, True])
def test_subpixel_kernel_and_the_operation_it_replaces(B, Cin, Cout, H, W, dtype, epi):
    """1. against the float64 2x2 convolutions of the same 16-bit operands (subpixel_weights(w) as rounded): fp32 accumulation, the only
    error is the rounding of the result — 2 EPS (1 + |ref|), the rule of test_conv3x3_nhwc.
    3. against the fp32 3x3 convolution of the upsampled input: |got - ref| <= EPS (S + 2 (1 + |ref|)), S = sum |W'_16| |x| — every summed
    weight is rounded once (relative error <= EPS each), which bounds the first term rigorously."""
    from sta import fused
    x, w, bias, res, wsub, ref2, ref3, S = _case(B, Cin, Cout, H, W, dtype)
    extra = (bias.double().view(1, -1, 1, 1) + res.double()) if epi else 0.0
    xd, wd = _nhwc(x), w.cuda()
    with torch.no_grad():
        assert fused.conv3x3_supported(xd, wd, up2=True) and fused.conv3x3_up2_subpixel_supported(xd, wd)
        got = fused.conv3x3_nhwc(xd, fused.pack_conv3x3_up2_weight(wd), Cout, up2=True, bias=bias.cuda() if epi else None,
                                 res=_nhwc(res) if epi else None, subpixel=True)
    torch.cuda.synchronize()
    assert got.shape == (B, Cout, H, W) and got.is_contiguous(memory_format=torch.channels_last)
    got = got.cpu().double()
    eps = EPS[dtype]
    r2 = ref2 + extra
    q2 = ((got - r2).abs() / (2.0 * eps * (1.0 + r2.abs()))).max().item()
    r3 = ref3.double() + extra
    q3 = ((got - r3).abs() / (eps * (S + 2.0 * (1.0 + r3.abs())))).max().item()
    print("kernel: %.3f of 2 EPS (1 + |ref|); vs 3x3: %.3f of EPS (S + 2 (1 + |ref|))" % (q2, q3))
    assert q2 <= 1.0, q2
    assert q3 <= 1.0, q3


@pytest.mark.parametrize("Cin,Cout", [(64, 160), (192, 320), (128, 256)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("w_nhwc", [False, True])
def test_subpixel_pack_layout(Cin, Cout, dtype, w_nhwc):
    """2. The packed image is subpixel_weights(w) as 1-KiB fragments [phase][part][channel step][u][v][tile t], lane (g, c) holding
    W'[16 nt part + 16 t + c][32 kc + 8 g .. + 7][u][v] — byte for byte (the kernel sums in the order the torch restatement does)."""
    from sta import fused
    g = torch.Generator().manual_seed(Cin + Cout)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).to(dtype)
    wd = _nhwc(w) if w_nhwc else w.cuda()
    packed = fused.pack_conv3x3_up2_weight(wd).cpu()
    nt = 10 if Cout % 160 == 0 else 8
    parts, nkc = Cout // (16 * nt), Cin // 32
    ws = fused.subpixel_weights(w).view(4, parts, nt, 16, nkc, 4, 8, 2, 2)       # [ph][part][t][c][kc][g][j][u][v]
    want = ws.permute(0, 1, 4, 7, 8, 2, 5, 3, 6).contiguous()                   # [ph][part][kc][u][v][t][g][c][j]
    assert packed.numel() == want.numel() * 2
    assert torch.equal(packed.view(torch.int16), want.view(torch.int16).reshape(-1))


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(1, 64, 160, 64, 64), (2, 192, 320, 32, 32), (3, 128, 320, 16, 16), (2, 64, 256, 64, 64)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_subpixel_epilogue_statistics_feed_the_groupnorm(B, Cin, Cout, H, W, dtype):
    """4. The four phases of a (tile, pixel quarter) store their partial sums in four slots; folded, they are the statistics of the stored
    tensor, and the GroupNorm that takes them equals the one that takes its own pass (the tolerances of
    test_conv3x3_epilogue_statistics_feed_the_groupnorm)."""
    from sta import fused
    x, w, bias, res, _, _, _, _ = _case(B, Cin, Cout, H, W, dtype)
    g = torch.Generator().manual_seed(B + Cin + Cout + H)
    gw = (1.0 + 0.2 * torch.randn(Cout, generator=g)).to(dtype).cuda()
    gb = (0.2 * torch.randn(Cout, generator=g)).to(dtype).cuda()
    add = torch.randn(B, Cout, generator=g).cuda()
    xd, bd, rd = _nhwc(x), bias.cuda(), _nhwc(res)
    with torch.no_grad():
        wp = fused.pack_conv3x3_up2_weight(w.cuda())
        y = fused.conv3x3_nhwc(xd, wp, Cout, up2=True, bias=bd, res=rd, stats=True, subpixel=True)
        plain = fused.conv3x3_nhwc(xd, wp, Cout, up2=True, bias=bd, res=rd, subpixel=True)
        assert torch.equal(y, plain) and not hasattr(plain, "_sta_stats")
        st = fused._producer_stats(y)
        yf = y.float()
        ref = torch.stack([yf.sum(dim=(2, 3)), (yf * yf).sum(dim=(2, 3))], dim=-1)
        assert st.shape == (B, Cout, 2)
        assert ((st - ref).abs() <= 2e-3 * ref.abs() + 2e-2).all(), (st - ref).abs().max().item()
        for a_ in (None, add):
            one = fused.groupnorm_silu(y, gw, gb, 32, 1e-5, add=a_)
            two = fused.groupnorm_silu(plain, gw, gb, 32, 1e-5, add=a_).float().cpu()
            err = (one.float().cpu() - two).abs()
            assert (err <= 2.0 * EPS[dtype] * (1.0 + two.abs())).all(), err.max().item()


def _module(Cin, Cout, dtype, seed=0):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(Cin, Cout, 3, padding=1).to(dtype).cuda()
    with torch.no_grad():
        conv.weight.mul_(3.0 / (9 * Cin) ** 0.5 / conv.weight.std())
    return conv


def _spy(monkeypatch, fused):
    calls = []
    real = fused.conv3x3_nhwc
    monkeypatch.setattr(fused, "conv3x3_nhwc", lambda *a, **k: (calls.append((k.get("up2", False), k.get("subpixel", False))), real(*a, **k))[1])
    return calls, real


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_switch_off_is_the_3x3_path(monkeypatch, dtype):
    """5. CONV_UP2_SUBPIXEL = False: the module result is bit-equal to the 3x3 `up2` kernel's; on: it is the sub-pixel launch's."""
    from sta import fused
    conv = _module(64, 160, dtype)
    x = _nhwc(torch.randn(2, 64, 16, 16).to(dtype))
    calls, real = _spy(monkeypatch, fused)
    with torch.no_grad():
        parent = real(x, fused.pack_conv3x3_weight(conv.weight), 160, up2=True, bias=conv.bias)
        sub = real(x, fused.pack_conv3x3_up2_weight(conv.weight), 160, up2=True, bias=conv.bias, subpixel=True)
        monkeypatch.setattr(fused, "CONV_UP2_SUBPIXEL", False)
        off = fused.conv3x3_module(conv, conv, x, bias=conv.bias, up2=True, stats=False)
        monkeypatch.setattr(fused, "CONV_UP2_SUBPIXEL", True)
        on = fused.conv3x3_module(conv, conv, x, bias=conv.bias, up2=True, stats=False)
    assert calls == [(True, False), (True, True)]
    assert torch.equal(off, parent) and torch.equal(on, sub)
    assert not torch.equal(on, off)              # (the two paths differ by the rounding of the summed weights)


def test_in_place_weight_update_repacks(monkeypatch):
    """6. The sub-pixel image is cached under a slot of its own; conv.weight.mul_(0.5) is followed by a repack."""
    from sta import fused
    conv = _module(64, 160, torch.float16)
    x = _nhwc(torch.randn(2, 64, 16, 16).half())
    packs = []
    real_pack = fused.pack_conv3x3_up2_weight
    monkeypatch.setattr(fused, "pack_conv3x3_up2_weight", lambda w: (packs.append(1), real_pack(w))[1])
    with torch.no_grad():
        a = fused.conv3x3_module(conv, conv, x, bias=conv.bias, up2=True, stats=False)
        a2 = fused.conv3x3_module(conv, conv, x, bias=conv.bias, up2=True, stats=False)
        assert len(packs) == 1 and torch.equal(a, a2)
        assert ("conv_up2", id(conv)) in conv._sta_images and ("conv", id(conv)) not in conv._sta_images
        conv.weight.mul_(0.5)
        b = fused.conv3x3_module(conv, conv, x, bias=conv.bias, up2=True, stats=False)
        assert len(packs) == 2
        want = fused.conv3x3_nhwc(x, real_pack(conv.weight), 160, up2=True, bias=conv.bias, subpixel=True)
    assert torch.equal(b, want) and not torch.equal(a, b)


def test_unsupported_low_resolution_geometry_stays_on_the_3x3_path(monkeypatch):
    """7. A 16-wide, 8-high input has no tile geometry of its own (its 32 x 16 output has one): the support query says no, the launch
    refuses, and the module takes the 3x3 kernel."""
    from sta import fused, lib
    conv = _module(64, 160, torch.float16)
    x = _nhwc(torch.randn(4, 64, 8, 16).half())
    L = lib.load()
    assert L.sta_conv3x3_nhwc_supported(4, 16, 32, 64, 160) and not L.sta_conv3x3_up2_nhwc_supported(4, 16, 32, 64, 160)
    assert not fused.conv3x3_up2_subpixel_supported(x, conv.weight)
    calls, real = _spy(monkeypatch, fused)
    with torch.no_grad():
        got = fused.conv3x3_module(conv, conv, x, bias=conv.bias, up2=True, stats=False)
        assert calls == [(True, False)]
        assert torch.equal(got, real(x, fused.pack_conv3x3_weight(conv.weight), 160, up2=True, bias=conv.bias))
        with pytest.raises(RuntimeError, match="unsupported geometry"):
            real(x, fused.pack_conv3x3_up2_weight(conv.weight), 160, up2=True, subpixel=True)


def test_batch_split_below_the_descriptor_limit(monkeypatch):
    """The batch split at CONV_MAX_BYTES works as for the 3x3 path (statistics slots of a chunk included)."""
    from sta import fused
    x, w, bias, res, _, _, _, _ = _case(3, 64, 160, 32, 32, torch.float16)
    xd, rd = _nhwc(x), _nhwc(res)
    with torch.no_grad():
        wp = fused.pack_conv3x3_up2_weight(w.cuda())
        one = fused.conv3x3_nhwc(xd, wp, 160, up2=True, res=rd, stats=True, subpixel=True)
        monkeypatch.setattr(fused, "CONV_MAX_BYTES", 2 * 32 * 32 * 160 * 2)       # two images per launch: 2 + 1
        split = fused.conv3x3_nhwc(xd, wp, 160, up2=True, res=rd, stats=True, subpixel=True)
    assert torch.equal(one, split) and torch.equal(fused._producer_stats(one), fused._producer_stats(split))
