"""sta_ln_qkv (csrc/sta_lnqkv.hip): norm1 + the q|k and V^T projections of level-0 self-attention as one pass — the kernel against
fp32, its refusals, and the full-width UNet with the pass on and off."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402

C = 320
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def _inputs(R, dtype, seed=0):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    # a per-row offset and a non-unit scale, so that the mean and the variance matter
    x = (rn(R, C) * 1.7 + rn(R, 1) * 3.0 + 0.5).to(dtype)
    bias = (rn(C) * 0.3).to(dtype)
    gamma = (1.0 + 0.2 * rn(C)).to(dtype)
    beta = (0.1 * rn(C)).to(dtype)
    wqk = (rn(2 * C, C) / C ** 0.5).to(dtype)
    wv = (rn(C, C) / C ** 0.5).to(dtype)
    return x, bias, gamma, beta, wqk, wv


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("R", [16, 4096 + 16, 65536, 524288])
def test_ln_qkv_kernel_vs_fp32(R, dtype, with_bias):
    """y (exported through y_dbg) and s are bit-identical to sta_add_layernorm's; q|k and V^T against the fp32 product of that y
    with the 16-bit weights, every element within 2 eps (1 + |ref|) (fp32 accumulation: the error is the rounding of the result)."""
    from sta import fused
    x, bias, gamma, beta, wqk, wv = _inputs(R, dtype, seed=R % 1000 + int(with_bias))
    b = bias if with_bias else None
    packed = fused.pack_ln_qkv_weight(wqk, wv)
    y_dbg = torch.full_like(x, float("nan"))
    s, qk, vt = fused.ln_qkv(x, b, gamma, beta, 1e-5, packed, store_sum=with_bias, y_dbg=y_dbg)
    s_ref, y_ref = fused.add_layernorm(x, None, b, gamma, beta, 1e-5, store_sum=with_bias)
    assert torch.equal(y_dbg, y_ref)
    if with_bias:
        assert torch.equal(s, s_ref)
    else:
        assert s is None
    assert qk.shape == (R, 2 * C) and vt.shape == (C, R)
    eps = EPS[dtype]
    worst = {}
    step = 65536                                   # the fp32 reference one slice of rows at a time
    for name, got_all, w in (("qk", qk, wqk), ("vt", vt.t(), wv)):
        m = 0.0
        for i in range(0, R, step):
            ref = F.linear(y_dbg[i:i + step].float(), w.float())
            got = got_all[i:i + step].float()
            assert torch.isfinite(got).all()
            m = max(m, ((got - ref).abs() / (eps * (1 + ref.abs()))).max().item())
        worst[name] = m
    print("ln_qkv R=%d %s bias=%s: max err / (eps (1 + |ref|)): qk %.3f vt %.3f" % (R, dtype, with_bias, worst["qk"], worst["vt"]))
    assert worst["qk"] <= 2.0 and worst["vt"] <= 2.0, worst


def test_ln_qkv_refusals():
    """C = 640, a row count that is not a multiple of 16, an output past 4 GiB: non-zero return, the reason in sta_last_error,
    outputs untouched; the Python gate then selects the row-major path."""
    from sta import fused, lib
    L = lib.load()
    dtype = torch.float16
    x, bias, gamma, beta, wqk, wv = _inputs(64, dtype)
    packed = fused.pack_ln_qkv_weight(wqk, wv)
    qk = torch.full((64, 2 * C), 7.0, dtype=dtype, device=x.device)
    vt = torch.full((C, 64), 7.0, dtype=dtype, device=x.device)
    st = torch.cuda.current_stream().cuda_stream

    def call(R, c):
        return L.sta_ln_qkv(x.data_ptr(), None, gamma.data_ptr(), beta.data_ptr(), packed.data_ptr(), None, None, qk.data_ptr(), vt.data_ptr(),
                            R, c, 1e-5, lib.STA_F16, st)
    assert L.sta_ln_qkv_packed_w_bytes(640) == 0 and L.sta_ln_qkv_packed_w_bytes(C) == 600 * 1024
    assert call(64, 640) != 0 and "C = 320 only" in lib.last_error()
    assert call(40, C) != 0 and "multiple of 16" in lib.last_error()
    big = (1 << 32) // (2 * C * 2) // 16 * 16 + 16
    assert call(big, C) != 0 and "4 GiB" in lib.last_error()
    assert L.sta_ln_qkv_pack_w(wqk.data_ptr(), wv.data_ptr(), packed.data_ptr(), 640, lib.STA_F16, st) != 0 and "C = 320 only" in lib.last_error()
    torch.cuda.synchronize()
    assert (qk == 7.0).all() and (vt == 7.0).all()
    assert fused.ln_qkv_supported(torch.empty(2, 32, C, dtype=dtype, device=x.device))
    assert not fused.ln_qkv_supported(torch.empty(2, 32, 640, dtype=dtype, device=x.device))
    assert not fused.ln_qkv_supported(torch.empty(1, 40, C, dtype=dtype, device=x.device))
    assert not fused.ln_qkv_supported(torch.empty(big, C, dtype=dtype, device="meta"))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_ln_qkv_graph_replay_is_bitwise_the_eager_result(dtype):
    from sta import fused
    x, bias, gamma, beta, wqk, wv = _inputs(8192, dtype, seed=3)
    packed = fused.pack_ln_qkv_weight(wqk, wv)
    s0, qk0, vt0 = fused.ln_qkv(x, bias, gamma, beta, 1e-5, packed)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused.ln_qkv(x, bias, gamma, beta, 1e-5, packed)        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s1, qk1, vt1 = fused.ln_qkv(x, bias, gamma, beta, 1e-5, packed)
    for t in (s1, qk1, vt1):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(s0, s1) and torch.equal(qk0, qk1) and torch.equal(vt0, vt1)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_full_width_unet_ln_qkv_on_vs_off(dtype, monkeypatch):
    """One CFG call of the full-width UNet (batch 2; ROWGEMM_MIN_ROWS lowered so that the five level-0 blocks take the fused chain at
    8192 rows) with fused.LN_QKV on and off. On: fused.ln_qkv runs exactly five times; off: never, and the five norm1
    add_layernorm passes come back. Outputs: fp16 max |diff| < 0.8 % of max |eps| (the bound of the in-place-concatenation test:
    a library GEMM replaced by ours), bf16 6 % / 2 % max / mean (the bound of the HIP-vs-library convolution test)."""
    from sta import fused, prompt_state
    from sta.pipeline import build_sd_v1, use_shipped_miopen_db
    use_shipped_miopen_db(0)
    dev = torch.device("cuda", 0)
    model = build_sd_v1(dev, dtype, with_vae=False, init_weights=True, seed=0, channels_last=True)
    unet = model.model.diffusion_model
    c, local_ctx, x = gi.unet_inputs(2, 6, lat=64)
    ctx = torch.cat([gi.load_uncond(), c]).to(dev, dtype)
    xin = x.expand(2, -1, -1, -1).contiguous().to(dev)
    t = torch.tensor([981, 981], device=dev)
    coef = torch.tensor([2.5, 2.5], device=dev)
    monkeypatch.setattr(fused, "ROWGEMM_MIN_ROWS", 8192)
    monkeypatch.setattr(fused, "CONV_MIN_ITEMS", 1)
    n = {"ln_qkv": 0, "add_layernorm": 0}
    real_q, real_l = fused.ln_qkv, fused.add_layernorm
    monkeypatch.setattr(fused, "ln_qkv", lambda *a, **k: (n.__setitem__("ln_qkv", n["ln_qkv"] + 1), real_q(*a, **k))[1])
    monkeypatch.setattr(fused, "add_layernorm", lambda *a, **k: (n.__setitem__("add_layernorm", n["add_layernorm"] + 1), real_l(*a, **k))[1])
    out, counts = {}, {}
    for on in (True, False):
        monkeypatch.setattr(fused, "LN_QKV", on)
        n["ln_qkv"] = n["add_layernorm"] = 0
        prompt_state.begin_prompt([l.to(dev) for l in local_ctx], first_timestep=981)
        with torch.no_grad():
            out[on] = unet(xin, 0, t, context=ctx, coef=coef, bboxs_curr=[[0.3, 0.4], [0.7, 0.6]]).float()
        counts[on] = dict(n)
    assert counts[True]["ln_qkv"] == 5 and counts[False]["ln_qkv"] == 0, counts
    assert counts[False]["add_layernorm"] == counts[True]["add_layernorm"] + 5, counts
    ref, got = out[False], out[True]
    assert torch.isfinite(got).all() and ref.abs().max() > 1e-2
    e_max = ((got - ref).abs().max() / ref.abs().max()).item()
    e_mean = ((got - ref).abs().mean() / ref.abs().mean()).item()
    print("full-width UNet, LN_QKV on vs off (%s): max %.5f mean %.5f (relative)" % (dtype, e_max, e_mean))
    if dtype == torch.float16:
        assert e_max < 0.008, (e_max, e_mean)
    else:
        assert e_max < 0.06 and e_mean < 0.02, (e_max, e_mean)
