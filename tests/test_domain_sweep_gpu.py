"""Every finite 16-bit input through the elementwise kernels: GELU inside sta_geglu, sta_geglu_bwd, the GEGLU projection passes
(csrc/sta_ffgemm.hip) and the MXFP8 GEMM epilogue, SiLU behind the GroupNorm kernels (every NCHW and NHWC instance, the concatenation and the
producer-statistics forms), and the two fp8 quantisers bit for bit at
power-of-two scales. References are fp64; the bounds, their derivation and the value operands V are in tests/sweep16.py, and
tests/test_domain_sweep_cpu.py shows that the bounds leave the kernels' formulas a factor of two and reject cheaper ones.
Every case prints its worst error / bound and where it occurred."""
import pytest
import torch

from tests import sweep16 as sw

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
D = 512


@pytest.fixture(autouse=True)
def _kernels_at_every_size(monkeypatch):
    """The product routes launches with few work items to the library (sta.fused.CONV_MIN_ITEMS); the sweeps run the kernels at tiny shapes."""
    from sta import fused
    monkeypatch.setattr(fused, "CONV_MIN_ITEMS", 1)


def _beyond_rounding(got, ref, bound_of, dtype):
    """How much of a bound's allowance for everything but the final rounding the result uses at the most: max of (err - u / 2) / (bound
    - u / 2). The figure the CPU emulations are held to 0.5 of (tests/test_domain_sweep_cpu.py); printed here, the assertion is the bound."""
    half_u = 0.5 * sw.ulp16(torch.maximum(got.double().abs(), ref.abs()), dtype)
    return float((((got.double() - ref).abs() - half_u).clamp(min=0.0) / bound_of(False)).max())


def _report(what, dtype, got, ref, bound_of, where):
    """`bound_of(rounding)`: the case's bound with or without its u / 2 term."""
    r, _, line = sw.worst(got, ref, bound_of(True), where)
    print("%s %s: %s; beyond the rounding: %.3f of the allowance" % (what, str(dtype).replace("torch.", ""), line,
                                                                      _beyond_rounding(got, ref, bound_of, dtype)))
    assert torch.isfinite(got.float()).all() and r <= 1.0, line


def _rows(flat, width):
    """A flat operand as [R, width] rows, the last row padded with repeats."""
    n = (flat.numel() + width - 1) // width * width
    return sw.tile_to(flat, n).view(-1, width)


@pytest.mark.parametrize("dtype", DTYPES)
def test_geglu_every_gate_and_every_value(dtype):
    """sta_geglu, h [R, 2 D] -> h[:, :D] * gelu(h[:, D:]) against v * gelu64(g) within geglu_fwd_bound: every gate at each v in V, every
    value at the gates 1, -1, 0.5, -3."""
    from sta import fused
    vals, gates = sw.geglu_operands(dtype)
    a, g = _rows(vals, D), _rows(gates, D)
    got = fused.geglu(torch.cat([a, g], dim=1).cuda()).cpu()
    ref = a.double() * sw.gelu64(g)
    _report("geglu", dtype, got, ref, lambda rnd: sw.geglu_fwd_bound(got, ref, a, g, dtype, rnd), {"v": a, "g": g})


@pytest.mark.parametrize("dtype", DTYPES)
def test_geglu_backward_every_gate(dtype):
    """sta_geglu_bwd through fused.geglu_tracked: every gate at each (dy, a) in V x V; dx's value half da = dy * gelu(g) within
    geglu_fwd_bound (v := dy), its gate half dg = dy * a * gelu'(g) within geglu_dgate_bound."""
    from sta import fused
    d = sw.domain(dtype)
    n = d.numel()
    dy = _rows(torch.cat([torch.full((n * len(sw.V),), v, dtype=dtype) for v in sw.V]), D)
    a = _rows(torch.cat([torch.full((n,), v, dtype=dtype) for v in sw.V] * len(sw.V)), D)
    g = _rows(torch.cat([d] * len(sw.V) ** 2), D)
    h = torch.cat([a, g], dim=1).cuda().requires_grad_(True)
    with fused.tracked():
        y = fused.geglu_tracked(h)
    assert "GegluFn" in type(y.grad_fn).__name__
    y.backward(dy.cuda())
    dx = h.grad.cpu()
    da, dg = dx[:, :D], dx[:, D:]
    where = {"dy": dy, "a": a, "g": g}
    ref = dy.double() * sw.gelu64(g)
    _report("geglu_bwd da", dtype, da, ref, lambda rnd, ref=ref: sw.geglu_fwd_bound(da, ref, dy, g, dtype, rnd), where)
    ref = dy.double() * a.double() * sw.gelu_grad64(g)
    _report("geglu_bwd dg", dtype, dg, ref, lambda rnd, ref=ref: sw.geglu_dgate_bound(dg, ref, dy, a, g, dtype, rnd), where)


def _ff_geglu_case(dtype, C, inner, R):
    """The GEGLU projection with a GEMM that contributes no error: the weight's value rows are zero and its gate row inner + j is
    one-hot at column j mod C; the bias is V[j // C] on the value half and 0 on the gate half. With y [R, C] holding the domain (padded
    with repeats) the output is h[r, j] = V[j // C] * gelu(y[r, j mod C]), the gate inside the kernel being y itself."""
    assert inner == len(sw.V) * C
    y = _rows(sw.domain(dtype), C)
    assert y.shape[0] <= R
    y = sw.tile_to(y.reshape(-1), R * C).view(R, C)
    j = torch.arange(inner)
    w = torch.zeros(2 * inner, C, dtype=dtype)
    w[inner + j, j % C] = 1.0
    bias = torch.zeros(2 * inner, dtype=dtype)
    bias[:inner] = torch.tensor(sw.V, dtype=torch.float64)[j // C].to(dtype)
    v = bias[:inner].view(1, inner).expand(R, inner)
    g = y.repeat(1, len(sw.V))
    return y, w, bias, v, g


@pytest.mark.parametrize("dtype", DTYPES)
def test_ff_geglu_qfrag_every_gate(dtype):
    """sta_ff_geglu_qfrag (C = 320, inner = 1280; ff_gelu_erf behind the MFMA accumulators): every 16-bit value as the gate of each v in
    V, within geglu_fwd_bound; h in fragment order holds the same values."""
    from sta import fused, ops
    C, inner, R = 320, 1280, 208
    y, w, bias, v, g = _ff_geglu_case(dtype, C, inner, R)
    wp = fused.pack_geglu_weight(w.cuda())
    yq = ops.to_qfrag(y.cuda())
    h = fused.ff_geglu_qfrag(yq, wp, bias.cuda(), inner)
    hf = fused.ff_geglu_qfrag(yq, wp, bias.cuda(), inner, h_frag=True)
    torch.cuda.synchronize()
    assert torch.equal(ops.from_qfrag(hf), h)
    got = h.cpu()
    ref = v.double() * sw.gelu64(g)
    _report("ff_geglu_qfrag", dtype, got, ref, lambda rnd: sw.geglu_fwd_bound(got, ref, v, g, dtype, rnd), {"v": v, "g": g})


@pytest.mark.parametrize("dtype", DTYPES)
def test_ff_geglu_c640_qfrag_every_gate(dtype):
    """sta_ff_geglu_c640_qfrag (C = 640, inner = 2560): the same sweep through the level-1 instance of the pass."""
    from sta import fused, ops
    C, inner, R = 640, 2560, 112
    y, w, bias, v, g = _ff_geglu_case(dtype, C, inner, R)
    wp = fused.pack_geglu_c640_weight(w.cuda())
    got = fused.ff_geglu_c640_qfrag(ops.to_qfrag(y.cuda()), wp, bias.cuda(), inner).cpu()
    ref = v.double() * sw.gelu64(g)
    _report("ff_geglu_c640_qfrag", dtype, got, ref, lambda rnd: sw.geglu_fwd_bound(got, ref, v, g, dtype, rnd), {"v": v, "g": g})


@pytest.mark.parametrize("dtype", DTYPES)
def test_mxfp8_geglu_epilogue_every_gate_and_every_value(dtype):
    """sta_mx8_gemm's GEGLU epilogue (libm erff) with 16-bit output: P is all code 0 at scale 2^0, so the accumulators are exactly 0 for
    any Q and value and gate are the bias alone (packed by pack_geglu_rows). Every gate at each v in V and every value at the gates
    1, -1, 0.5, -3, in one launch of M = 5 rows, K = 32; the five rows must agree bit for bit."""
    from sta import mxfp8
    vals, gates = sw.geglu_operands(dtype)
    H = (vals.numel() + 31) // 32 * 32
    vals, gates = sw.tile_to(vals, H), sw.tile_to(gates, H)
    N, M, K = 2 * H, 5, 32
    gen = torch.Generator().manual_seed(16)
    q = (torch.randn(N, K, generator=gen) * 8).clamp(-448, 448).to(torch.float8_e4m3fn)
    qs = torch.randint(123, 128, (N, 1), generator=gen, dtype=torch.uint8)
    p = torch.zeros(M, K, dtype=torch.uint8).view(torch.float8_e4m3fn)
    ps = torch.full((M, 1), 127, dtype=torch.uint8)
    perm = mxfp8.pack_geglu_rows(N)
    bias = torch.cat([vals, gates])[perm]
    out = mxfp8.gemm(p.cuda(), ps.cuda(), q.cuda(), qs.cuda(), dtype, bias=bias.cuda(), geglu=True)
    assert out.shape == (M, H)
    assert (out.view(torch.int16) == out[:1].view(torch.int16)).all()
    got = out[0].cpu()
    ref = vals.double() * sw.gelu64(gates)
    _report("mxfp8 geglu epilogue", dtype, got, ref, lambda rnd: sw.geglu_fwd_bound(got, ref, vals, gates, dtype, rnd), {"v": vals, "g": gates})


# ---------------------------------------------------------------------------------------------------------------------------------
# SiLU behind GroupNorm: gamma = 0 and beta = a slice of the domain. The kernels form z = x * (gamma rstd) + (beta - mean gamma rstd),
# so z = beta for any finite x: every pixel of channel c is silu(beta_c), and with silu=False it is beta_c itself.
# One place is not pinned bit for bit: beta = -0. IEEE addition gives (-0) + (+0) = +0, and x * 0 and mean * 0 carry the signs of x
# and of the mean, so z is +0 or -0 from pixel to pixel there (the value, 0, is exact). The sweeps therefore compare bits everywhere
# except that a zero may be either zero at the one channel whose beta is -0.
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16)


def _silu_sweep(what, dtype, C, launch):
    """`launch(beta [C] cuda, silu) -> y [B, C, H, W]` over the domain in slices of C channels (the last padded with repeats)."""
    d = sw.domain(dtype)
    betas = _rows(d, C)
    worst_r, worst_line, beyond = 0.0, "", 0.0
    for beta in betas:
        bc = beta.cuda()
        for silu in (True, False):
            y = launch(bc, silu)
            assert y.shape[1] == C
            ych = y.permute(1, 0, 2, 3).reshape(C, -1)                          # [C, pixels] (a view of either memory format)
            first = ych[:, :1]
            same = (_bits(ych) == _bits(first)) | ((ych == 0) & (first == 0) & (bc == 0).view(C, 1))
            assert same.all(), "%s: pixels of one channel differ, e.g. beta = %r" % (what, float(bc[(~same).any(dim=1)][0]))
            got = first.reshape(C).cpu()
            assert torch.isfinite(got.float()).all(), "%s silu=%s: not finite at beta = %r" % (what, silu, float(beta[~torch.isfinite(got.float())][0]))
            if silu:
                ref = sw.silu64(beta)
                r, _, line = sw.worst(got, ref, sw.silu_bound(got, ref, beta, dtype), {"z": beta})
                if r >= worst_r:
                    worst_r, worst_line = r, line
                beyond = max(beyond, _beyond_rounding(got, ref, lambda rnd: sw.silu_bound(got, ref, beta, dtype, rnd), dtype))
            else:
                plain = (_bits(got) == _bits(beta)) | ((got == 0) & (beta == 0))
                assert plain.all(), "%s silu=False: got %r for beta = %r" % (what, float(got[~plain][0]), float(beta[~plain][0]))
    print("%s %s: %s; beyond the rounding: %.3f of the allowance" % (what, str(dtype).replace("torch.", ""), worst_line, beyond))
    assert worst_r <= 1.0, worst_line


def _x(shape, dtype, nhwc, seed=0):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()
    return x.contiguous(memory_format=torch.channels_last) if nhwc else x


# the four instances of gn_silu_kernel that keep the slab in registers (gn_dispatch, csrc/sta_unet.hip: by the slab's 16-byte vectors,
# 64 channels x H W / 8 here): <256, 2> up to 512 vectors, <256, 8> up to 2048, <1024, 4> up to 4096, <1024, 8> up to 8192
@pytest.mark.parametrize("H,W", [(4, 4), (8, 16), (16, 24), (24, 32)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_behind_groupnorm_nchw_registers(dtype, H, W):
    """sta_groupnorm_silu with the (b, group) slab in registers: C = 2048, G = 32, slabs of 128, 1024, 3072 and 6144 vectors."""
    from sta import fused
    C = 2048
    x, gamma = _x((1, C, H, W), dtype, False), torch.zeros(C, dtype=dtype, device="cuda")
    _silu_sweep("groupnorm_silu nchw registers %dx%d" % (H, W), dtype, C, lambda beta, silu: fused.groupnorm_silu(x, gamma, beta, 32, 1e-5, silu=silu))


@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_behind_groupnorm_nchw_two_pass(dtype):
    """sta_groupnorm_silu's two-pass kernel: slabs above 65536 elements (C = 8192, G = 32, 12 x 22: 67584 per slab)."""
    from sta import fused
    C = 8192
    # 8448 vectors: past the 1024 * 8 that gn_dispatch (csrc/sta_unet.hip) still gives to a register instance. The figure is a copy of
    # that threshold: if the dispatch moves, this shape has to move with it.
    assert (C // 32) * 12 * 22 // 8 > 1024 * 8
    x, gamma = _x((1, C, 12, 22), dtype, False), torch.zeros(C, dtype=dtype, device="cuda")
    _silu_sweep("groupnorm_silu nchw two-pass", dtype, C, lambda beta, silu: fused.groupnorm_silu(x, gamma, beta, 32, 1e-5, silu=silu))


# both instances of gn_nhwc_apply_kernel (gn_nhwc_apply_launch, csrc/sta_unet.hip: by the pixels a thread has, 10 or more take the
# streaming <4, true>): 4 x 4 gives a thread 8 pixels (<2, false>), 32 x 32 gives it 32
@pytest.mark.parametrize("H", [4, 32])
@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_behind_groupnorm_nhwc(dtype, H):
    """sta_groupnorm_silu_nhwc (statistics pass + apply pass): C = 2560, G = 32, two images, short and long trips."""
    from sta import fused
    C = 2560
    x, gamma = _x((2, C, H, H), dtype, True), torch.zeros(C, dtype=dtype, device="cuda")
    assert fused.is_nhwc(x)
    _silu_sweep("groupnorm_silu nhwc %dx%d" % (H, H), dtype, C, lambda beta, silu: fused.groupnorm_silu(x, gamma, beta, 32, 1e-5, silu=silu))


@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_behind_groupnorm_of_a_concatenation(dtype):
    """sta_groupnorm_silu_nhwc_cat: two NHWC tensors read in place (1280 + 640 channels in groups of 60: one group straddles the seam)."""
    from sta import fused
    Ca, Cb = 1280, 640
    xa, xb = _x((2, Ca, 4, 4), dtype, True, 1), _x((2, Cb, 4, 4), dtype, True, 2)
    gamma = torch.zeros(Ca + Cb, dtype=dtype, device="cuda")
    _silu_sweep("groupnorm_silu_cat", dtype, Ca + Cb, lambda beta, silu: fused.groupnorm_silu_cat(xa, xb, gamma, beta, 32, 1e-5, silu=silu))


@pytest.mark.parametrize("dtype", DTYPES)
def test_silu_behind_groupnorm_with_producer_statistics(dtype):
    """sta_groupnorm_silu_nhwc_cstats as the UNet reaches it: the tensor comes out of conv3x3_nhwc(..., stats=True) carrying its channel
    sums, and groupnorm_silu takes them instead of a statistics pass (Cout = 1280, G = 32, 8 x 8, two images)."""
    from sta import fused
    Cin, Cout = 64, 1280
    g = torch.Generator().manual_seed(3)
    x = _x((2, Cin, 8, 8), dtype, True, 3)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).to(dtype).cuda()
    gamma = torch.zeros(Cout, dtype=dtype, device="cuda")
    with torch.no_grad():
        y = fused.conv3x3_nhwc(x, fused.pack_conv3x3_weight(w), Cout, stats=True)
    assert fused._producer_stats(y) is not None and fused.is_nhwc(y)

    def launch(beta, silu):
        assert fused._producer_stats(y) is not None                        # still the one-pass form
        return fused.groupnorm_silu(y, gamma, beta, 32, 1e-5, silu=silu)
    _silu_sweep("groupnorm_silu producer statistics", dtype, Cout, launch)


# ---------------------------------------------------------------------------------------------------------------------------------
# the fp8 quantisers at power-of-two scales: the multiply by 1 / scale is exact there, so every code is pinned
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, -6])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quant_rows_fp8_codes_at_power_of_two_scales(dtype, k):
    """sta_quant_rows_fp8: rows of C = 5120 holding every 16-bit value with |x| <= 448 * 2^k and one element equal to 448 * 2^k. The
    scale must be 2^k exactly and every code must equal (x / 2^k).to(float8_e4m3fn) bit for bit: ties to even, e4m3 subnormals, +-0."""
    from sta import fp8
    C = 5120
    top = 448.0 * 2.0 ** k
    d = sw.domain(dtype)
    inside = d[d.double().abs() <= top]
    assert (inside.double() == top).sum() == 1                                    # 448 * 2^k is a value of both types
    x = _rows(inside, C - 1)
    x = torch.cat([torch.full((x.shape[0], 1), top, dtype=dtype), x], dim=1).contiguous()
    xq, scale = fp8.quant_rows(x.cuda())
    torch.cuda.synchronize()
    assert (scale.cpu() == 2.0 ** k).all(), scale.flatten().tolist()
    want = (x.float() / 2.0 ** k).to(torch.float8_e4m3fn).view(torch.uint8)
    got = xq.cpu().view(torch.uint8)
    bad = (got != want).nonzero()
    print("quant_rows_fp8 %s k=%d: %d inputs in %d rows, %d codes differ" % (str(dtype).replace("torch.", ""), k, inside.numel(), x.shape[0], bad.shape[0]))
    assert bad.numel() == 0, "%d codes differ, first: x = %r got 0x%02x want 0x%02x" % (
        bad.shape[0], x[tuple(bad[0])].item(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())


@pytest.mark.parametrize("dtype", DTYPES)
def test_quant_rows_mx_codes_at_pinned_block_maxima(dtype):
    """sta_mx8_quant_rows: 32-element blocks whose maximum is 448, 256 and the largest 16-bit value not above 511 (511 in fp16, 510 in bf16:
    X = 2^0, quotients in (448, 511] saturate), and the same times 2^-6; the other 31 slots walk every domain value not above the block
    maximum. Scales and codes bit for bit against quant_rows_mx_reference."""
    from sta import mxfp8
    d = sw.domain(dtype)
    da = d.double().abs()
    blocks = []
    for k in (0, -6):
        for m in (448.0, 256.0, float(da[da <= 511.0].max())):
            top = m * 2.0 ** k
            assert (da == top).any()
            body = _rows(d[da <= top], 31)
            blocks.append(torch.cat([torch.full((body.shape[0], 1), top, dtype=dtype), body], dim=1))
    blocks = torch.cat(blocks)
    blocks = torch.cat([blocks[:, 5:], blocks[:, :5]], dim=1)                       # the maximum sits at slot 27, not at a block's first
    K = 320
    x = _rows(blocks.reshape(-1), K)
    q, s = mxfp8.quant_rows_mx(x.cuda())
    torch.cuda.synchronize()
    rq, rs = mxfp8.quant_rows_mx_reference(x)
    assert set(rs.unique().tolist()) == {127, 121}
    assert torch.equal(s.cpu(), rs)
    got, want = q.cpu().view(torch.uint8), rq.view(torch.uint8)
    bad = (got != want).nonzero()
    print("quant_rows_mx %s: %d blocks, %d codes differ" % (str(dtype).replace("torch.", ""), x.numel() // 32, bad.shape[0]))
    assert bad.numel() == 0, "%d codes differ, first: x = %r got 0x%02x want 0x%02x" % (
        bad.shape[0], x[tuple(bad[0])].item(), got[tuple(bad[0])].item(), want[tuple(bad[0])].item())
