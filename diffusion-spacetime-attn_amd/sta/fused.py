"""Python face of include/sta_unet.h: one-pass HIP kernels for the elementwise / normalisation chains of the
UNet trunk around the cross-attention path (ResBlock, SpatialTransformer, BasicTransformerBlock, GEGLU).

The forward kernels are used for inference: `usable()` is False whenever autograd is recording, and the modules then run
the reference's eager sequence (which is also what the CPU tests exercise). `fused.ENABLED = False` (tools/, tests) switches
them off. For the tracked (weight-optimisation) epochs the same forward kernels are wrapped in autograd Functions whose
backward is a HIP input-gradient kernel (csrc/sta_unet_bwd.hip: parameters are frozen, only d(input) exists): `tracked_usable()`,
`GroupNormSiLUFn`, `GegluFn`, `AddLayerNormFn`, `AddBiasFn`. They are opt-in (`with fused.tracked():`, entered by PLMSSampler
around a tracked epoch under the per-call recomputation policy of sta.pipeline.set_recompute) so that the other policies keep
the eager chain the goldens pin."""

import torch

from . import lib

_DT = {torch.bfloat16: lib.STA_BF16, torch.float16: lib.STA_F16}
ENABLED = True          # A/B switch for tools/ and tests; nothing reads the environment
_hold = 0               # > 0 inside `held()`: the forward of a block that will be re-run under autograd
TRACKED = False         # differentiable fused glue ops while autograd records (see module docstring)


class held:
    """Context in which the inference-only kernels (this module, HIP self-attention) are not used although
    autograd is off: the no-grad forward of a recomputed block must run the SAME op chain as its re-run in
    backward, otherwise gradients are taken at activations the forward never produced (util._Recompute)."""

    def __enter__(self):
        global _hold
        _hold += 1

    def __exit__(self, *exc):
        global _hold
        _hold -= 1


class tracked:
    """Context in which the differentiable fused glue ops are used while autograd records (tracked epochs)."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        global TRACKED
        self.prev, TRACKED = TRACKED, self.on
        return self

    def __exit__(self, *exc):
        global TRACKED
        TRACKED = self.prev


def is_nhwc(x):
    """A 4-D activation stored channels_last (NHWC in memory) and not also plain-contiguous."""
    return x.dim() == 4 and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)


def usable(x):
    """Fused trunk kernels apply to dense (NCHW- or NHWC-contiguous) 16-bit CUDA activations outside autograd."""
    return (x.is_cuda and x.dtype in _DT and not torch.is_grad_enabled() and (x.is_contiguous() or is_nhwc(x))
            and ENABLED and not _hold)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def groupnorm_silu(x, weight, bias, groups, eps, add=None, silu=True):
    """act(GroupNorm(x + add[:, :, None, None])); x [B, C, *spatial] contiguous, add [B, C] or None."""
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C)
    if add is not None:
        add = add.float().contiguous()
        assert add.shape == (B, C)
    def eager():                                # shapes outside the kernels' limits: the reference's op chain
        h = x if add is None else x + add.to(x.dtype)[:, :, None, None]
        h = torch.nn.functional.group_norm(h, groups, weight, bias, eps)
        return torch.nn.functional.silu(h) if silu else h
    y = torch.empty_like(x)                     # keeps the memory format
    if is_nhwc(x):
        L = lib.load()
        if C % 8 or (C // groups < 8 and C // groups != 4) or C > 4096 or groups > 64:
            return eager()
        st = _producer_stats(x) if GN_STATS_FROM_PRODUCER else None
        if st is not None:
            # the kernel that wrote x accumulated every channel's sum and sum of squares (sta_conv3x3_nhwc / sta_linear_rows_stats): one pass
            lib.check(L.sta_groupnorm_silu_nhwc_cstats(x.data_ptr(), None, C, st.data_ptr(), None, _ptr(add), weight.data_ptr(), bias.data_ptr(),
                                                       y.data_ptr(), B, C, HW, groups, float(eps), int(bool(silu)), _DT[x.dtype], _stream()),
                      "sta_groupnorm_silu_nhwc_cstats")
            return y
        ws = torch.empty(L.sta_groupnorm_nhwc_workspace_bytes(B, HW, groups) // 4, dtype=torch.float32, device=x.device)
        lib.check(L.sta_groupnorm_silu_nhwc(x.data_ptr(), _ptr(add), weight.data_ptr(), bias.data_ptr(), y.data_ptr(),
                                            ws.data_ptr(), B, C, HW, groups, float(eps), int(bool(silu)), _DT[x.dtype], _stream()),
                  "sta_groupnorm_silu_nhwc")
        return y
    if HW % 8 or C % groups:
        return eager()
    lib.check(lib.load().sta_groupnorm_silu(x.data_ptr(), _ptr(add), weight.data_ptr(), bias.data_ptr(), y.data_ptr(),
                                            B, C, HW, groups, float(eps), int(bool(silu)), _DT[x.dtype], _stream()),
              "sta_groupnorm_silu")
    return y


def geglu(h):
    """h [..., 2D] -> h[..., :D] * gelu(h[..., D:])."""
    D = h.shape[-1] // 2
    if D % 8:
        a, gate = h.chunk(2, dim=-1)
        return a * torch.nn.functional.gelu(gate)
    y = torch.empty(*h.shape[:-1], D, dtype=h.dtype, device=h.device)
    lib.check(lib.load().sta_geglu(h.data_ptr(), y.data_ptr(), h.numel() // (2 * D), D, _DT[h.dtype], _stream()), "sta_geglu")
    return y


def add_layernorm(x, f, bias, ln_weight, ln_bias, eps, store_sum=True, qfrag=False):
    """s = x + f + bias; returns (s, LayerNorm(s)); f / bias may be None; s is None if store_sum is False.
    `qfrag`: y comes back in QUERY-FRAGMENT order (sta_add_layernorm_qfrag: same shape and bytes, 16-row groups as 1-KiB MFMA
    operand fragments) for sta.ops.xattn_forward_proj(..., qfrag=True), its only legal consumer."""
    C = x.shape[-1]
    if qfrag:
        if C % 32 or C > 1024 or (x.numel() // C) % 16:
            raise ValueError("query-fragment order needs C %% 32 == 0, C <= 1024 and a multiple of 16 rows, got %s" % (tuple(x.shape),))
        s = torch.empty_like(x) if store_sum else None
        y = torch.empty_like(x)
        lib.check(lib.load().sta_add_layernorm_qfrag(x.data_ptr(), _ptr(f), _ptr(bias), ln_weight.data_ptr(), ln_bias.data_ptr(),
                                                     _ptr(s), y.data_ptr(), x.numel() // C, C, float(eps), _DT[x.dtype], _stream()),
                  "sta_add_layernorm_qfrag")
        return s, y
    if C % 8 or C > 2048:
        t = x if f is None else x + f
        t = t if bias is None else t + bias
        return (t if store_sum else None), torch.nn.functional.layer_norm(t, (C,), ln_weight, ln_bias, eps)
    s = torch.empty_like(x) if store_sum else None
    y = torch.empty_like(x)
    lib.check(lib.load().sta_add_layernorm(x.data_ptr(), _ptr(f), _ptr(bias), ln_weight.data_ptr(), ln_bias.data_ptr(),
                                           _ptr(s), y.data_ptr(), x.numel() // C, C, float(eps), _DT[x.dtype], _stream()),
              "sta_add_layernorm")
    return s, y


FRAG_XATTN, FRAG_SELFATTN = 0, 1       # whose out-fragment order the packed weight's k-slots follow


def pack_to_out_weight(weight, heads, kind=FRAG_XATTN):
    """to_out.weight [C, C] -> the fragment image sta_to_out_ln_ofrag streams through LDS (uint8 tensor); once per model.
    `kind`: the producer of the activations it will multiply — the cross-attention kernel (attn2.to_out) or the self-attention
    kernel (attn1.to_out); their out-fragment orders differ."""
    C = weight.shape[0]
    L = lib.load()
    n = L.sta_to_out_ln_packed_wo_bytes(C, heads)
    if n == 0 or weight.shape != (C, C) or not weight.is_cuda:
        raise ValueError("to_out + LayerNorm in out-fragment order: a square CUDA weight with C = 320, 8 heads; got %s heads=%d" % (tuple(weight.shape), heads))
    w = weight.detach().contiguous()
    buf = torch.empty(n, dtype=torch.uint8, device=w.device)
    lib.check(L.sta_to_out_ln_pack_wo(w.data_ptr(), buf.data_ptr(), C, heads, int(kind), _DT[w.dtype], _stream()), "sta_to_out_ln_pack_wo")
    return buf


def to_out_add_layernorm_ofrag(x, blended_ofrag, wo_packed, bias, ln_weight, ln_bias, eps, heads=8, y_qfrag=False):
    """s = x + blended . W_o^T + bias; returns (s, LayerNorm(s)) — `blended_ofrag` in the out-fragment order of the kernel that
    produced it (sta.ops.xattn_forward_proj(..., ofrag=True) or sta.ops.self_attention(..., sfrag=True); `wo_packed` packed for
    that kind); to_out's result never exists in HBM (csrc/sta_rowgemm.hip). `y_qfrag`: LayerNorm(s) comes back in query-fragment
    order (as add_layernorm(..., qfrag=True))."""
    C = x.shape[-1]
    R = x.numel() // C
    x = x.contiguous()
    s, y = torch.empty_like(x), torch.empty_like(x)
    lib.check(lib.load().sta_to_out_ln_ofrag(blended_ofrag.data_ptr(), wo_packed.data_ptr(), _ptr(bias), x.data_ptr(), ln_weight.data_ptr(),
                                             ln_bias.data_ptr(), s.data_ptr(), y.data_ptr(), R, C, heads, float(eps), int(bool(y_qfrag)), _DT[x.dtype], _stream()),
              "sta_to_out_ln_ofrag")
    return s, y


# Rows from which the persistent row-GEMM passes (to_out + LayerNorm: 128 rows per workgroup pass; GEGLU projection: 256) fill the
# chip: below it the library GEMM + the separate pass are taken (8 prompts per UNet call at 512^2 = 65536 rows at level 0).
ROWGEMM_MIN_ROWS = 65536


def _version(t):
    """t._version, or None for tensors without a version counter (tensors created under torch.inference_mode() raise on the
    attribute): without one an in-place update cannot be noticed, so nothing that depends on it is cached or trusted."""
    try:
        return t._version
    except RuntimeError:
        return None


def cached_image(owner, slot, weights, build):
    """The image `build()` makes of `weights` (a packed, concatenated or mirrored copy a kernel streams), kept on `owner` under `slot`
    and rebuilt only when one of the weight tensors changed: another storage, an in-place update (version counter) or another
    dtype. THE repack rule of every packed-weight cache. A weight without a version counter (inference tensors, `_version`) keys
    with None: such tensors cannot be updated in place, so storage and dtype identify them."""
    key = tuple((w.data_ptr(), _version(w), w.dtype) for w in weights)
    images = owner.__dict__.setdefault("_sta_images", {})
    hit = images.get(slot)
    if hit is None or hit[0] != key:
        hit = images[slot] = (key, build())
    return hit[1]


def _producer_stats(x):
    """The per-channel sums the producing kernel left on `x` — only while x still holds what that kernel wrote (an in-place update
    since then bumps the tensor's version and the sums are ignored: the consumer then takes its own statistics pass)."""
    st = getattr(x, "_sta_stats", None)
    v = _version(x)
    return st[1] if st is not None and v is not None and st[0] == v else None


ROWGEMM_MAX_BYTES = 0xfffffff0 - 1     # what one launch of these passes addresses per tensor (32-bit buffer offsets)


def rows_addressable(x, width=None):
    """The row passes of csrc/sta_rowgemm.hip / sta_ffgemm.hip address every [rows, width] tensor of a launch through one 32-bit
    buffer descriptor and refuse rows * width * itemsize >= 4 GiB (`width`: the widest tensor of the chain, default x's own — the
    GEGLU output is [rows, 1280] at C = 320: 205 prompts per step at 512^2, 52 at 1024^2). The gate belongs in FRONT of the chain:
    once a producer has written fragment order there is no row-major fallback for its consumer."""
    rows = x.numel() // x.shape[-1]
    return rows * max(x.shape[-1], width or 0) * x.element_size() <= ROWGEMM_MAX_BYTES


def rowgemm_worthwhile(x, width=None):
    return x.numel() // x.shape[-1] >= ROWGEMM_MIN_ROWS and rows_addressable(x, width)


def _pack_ff_weight(weight, C, inner, bytes_symbol, pack_symbol, expected):
    """A feed-forward weight -> the fragment image its pass streams through LDS (uint8 tensor); once per model. `expected`: what the
    ValueError says the pass takes."""
    L = lib.load()
    n = getattr(L, bytes_symbol)(C, inner)
    if n == 0 or not weight.is_cuda:
        raise ValueError("%s; got %s" % (expected, tuple(weight.shape)))
    w = weight.detach().contiguous()
    buf = torch.empty(n, dtype=torch.uint8, device=w.device)
    lib.check(getattr(L, pack_symbol)(w.data_ptr(), buf.data_ptr(), C, inner, _DT[w.dtype], _stream()), pack_symbol)
    return buf


def _ff_geglu(symbol, y_qfrag, w_packed, bias, inner, option):
    """One GEGLU projection pass (csrc/sta_ffgemm.hip); `option`: the entry point's one integer (h_frag | max_workgroups)."""
    C = y_qfrag.shape[-1]
    R = y_qfrag.numel() // C
    h = torch.empty(*y_qfrag.shape[:-1], inner, dtype=y_qfrag.dtype, device=y_qfrag.device)
    lib.check(getattr(lib.load(), symbol)(y_qfrag.data_ptr(), w_packed.data_ptr(), _ptr(bias), h.data_ptr(), R, C, inner, option,
                                          _DT[y_qfrag.dtype], _stream()), symbol)
    return h


def pack_geglu_weight(weight):
    """GEGLU proj.weight [2 * inner, C] -> the fragment image sta_ff_geglu_qfrag streams through LDS (uint8 tensor); once per model."""
    two_inner, C = weight.shape
    return _pack_ff_weight(weight, C, two_inner // 2, "sta_ff_geglu_packed_w_bytes", "sta_ff_geglu_pack_w", "fused GEGLU projection: a CUDA weight [2560, 320]")


def ff_geglu_supported(C, inner):
    return bool(lib.load().sta_ff_geglu_packed_w_bytes(C, inner))


def ff_geglu_qfrag(y_qfrag, w_packed, bias, inner, h_frag=False):
    """h = (y W_v^T + b_v) * gelu(y W_g^T + b_g) with y in query-fragment order ([.., C] container); returns h [.., inner], row-major
    or (`h_frag`) in the fragment order ff_out_res_hfrag reads. The [.., 2 * inner] projection never exists in HBM (csrc/sta_ffgemm.hip)."""
    return _ff_geglu("sta_ff_geglu_qfrag", y_qfrag, w_packed, bias, inner, int(bool(h_frag)))


FF_GEGLU_C640 = True    # level 1 (C = 640): the GEGLU projection + gelu * mul as one pass (csrc/sta_ffgemm.hip); False: library GEMM + sta_geglu


def pack_geglu_c640_weight(weight):
    """GEGLU proj.weight [5120, 640] -> the fragment image sta_ff_geglu_c640_qfrag streams through LDS (uint8 tensor); once per model."""
    two_inner, C = weight.shape
    return _pack_ff_weight(weight, C, two_inner // 2, "sta_ff_geglu_c640_packed_w_bytes", "sta_ff_geglu_c640_pack_w", "fused GEGLU projection (c640): a CUDA weight [5120, 640]")


def ff_geglu_c640_supported(C, inner):
    return bool(lib.load().sta_ff_geglu_c640_packed_w_bytes(C, inner))


def ff_geglu_c640_qfrag(y_qfrag, w_packed, bias, inner, max_workgroups=0):
    """ff_geglu_qfrag at C = 640, inner = 2560; h [.., inner] row-major. `max_workgroups` > 0 caps the grid (tests: several passes per
    persistent workgroup at a small row count)."""
    return _ff_geglu("sta_ff_geglu_c640_qfrag", y_qfrag, w_packed, bias, inner, int(max_workgroups))


def pack_ff_out_weight(weight):
    """FeedForward net[2].weight [C, inner] -> the fragment image sta_ff_out_res_hfrag streams through LDS; once per model."""
    C, inner = weight.shape
    return _pack_ff_weight(weight, C, inner, "sta_ff_out_packed_w_bytes", "sta_ff_out_pack_w", "fused feed-forward output: a CUDA weight [320, 1280]")


def ff_out_res_hfrag(x, h_frag, w_packed, bias):
    """x + h W2^T + b2 with h in fragment order (ff_geglu_qfrag(..., h_frag=True)); one pass (csrc/sta_ffgemm.hip)."""
    C, inner = x.shape[-1], h_frag.shape[-1]
    R = x.numel() // C
    x = x.contiguous()
    out = torch.empty_like(x)
    lib.check(lib.load().sta_ff_out_res_hfrag(h_frag.data_ptr(), w_packed.data_ptr(), _ptr(bias), x.data_ptr(), out.data_ptr(), R, C, inner,
                                              _DT[x.dtype], _stream()), "sta_ff_out_res_hfrag")
    return out


TO_OUT_LN_C640 = True   # level 1 (C = 640): attn1 / attn2 .to_out + the residual + the next LayerNorm as one pass (csrc/sta_rows640.hip); False: library GEMM + sta_add_layernorm
FF_OUT_RES_C640 = True  # level 1: ff.net[2] + the block's last residual as one pass (the same kernel at K = 2560); False: library GEMM + an elementwise add


def rows_c640_supported(x, lin):
    """`lin` is a plain nn.Linear [640 <- 640 | 2560] of x's dtype on x's device, x [.., 640] has a multiple of 16 rows, and the
    [rows, in_features] input stays below what a launch addresses."""
    C = x.shape[-1]
    return (type(lin) is torch.nn.Linear and lin.weight.dtype == x.dtype and lin.weight.is_cuda and lin.out_features == C
            and (x.numel() // C) % 16 == 0 and rows_addressable(x, lin.in_features)
            and bool(lib.load().sta_rows_c640_packed_w_bytes(C, lin.in_features)))


def pack_rows_c640_weight(weight):
    """A Linear weight [640, K] (K = 640 | 2560) -> the fragment image sta_rows_c640 streams through LDS (uint8 tensor); once per model."""
    C, K = weight.shape
    return _pack_ff_weight(weight, C, K, "sta_rows_c640_packed_w_bytes", "sta_rows_c640_pack_w", "Linear + residual at C = 640: a CUDA weight [640, 640] or [640, 2560]")


def rows_c640(x, a, w_packed, bias, ln_weight=None, ln_bias=None, eps=1e-5, y_qfrag=False, max_workgroups=0):
    """s = x + a W^T + bias over row-major a [.., K] and x [.., 640]; with `ln_weight` (K = 640) also y = LayerNorm(s), row-major or
    (`y_qfrag`) in query-fragment order. Returns (s, y); y is None without the LayerNorm (K = 2560). The Linear's result never exists
    in HBM (csrc/sta_rows640.hip). `max_workgroups` > 0 caps the grid (tests)."""
    C, K = x.shape[-1], a.shape[-1]
    R = x.numel() // C
    if a.numel() // K != R or a.dtype != x.dtype:
        raise ValueError("rows_c640: a %s and x %s must have the same rows and dtype" % (tuple(a.shape), tuple(x.shape)))
    x, a = x.contiguous(), a.contiguous()
    s = torch.empty_like(x)
    y = torch.empty_like(x) if ln_weight is not None else None
    lib.check(lib.load().sta_rows_c640(a.data_ptr(), w_packed.data_ptr(), _ptr(bias), x.data_ptr(), _ptr(ln_weight), _ptr(ln_bias), s.data_ptr(), _ptr(y),
                                       R, C, K, float(eps), int(bool(y_qfrag)), int(max_workgroups), _DT[x.dtype], _stream()), "sta_rows_c640")
    return s, y


def linear_res_c640(x, a, lin, norm=None, y_qfrag=False):
    """x + lin(a) (and norm of it) for a Linear rows_c640_supported accepted; the packed weight is cached on `lin`."""
    w = lin.weight
    wp = cached_image(lin, "rows_c640", (w,), lambda: pack_rows_c640_weight(w))
    if norm is None:
        return rows_c640(x, a, wp, lin.bias)
    return rows_c640(x, a, wp, lin.bias, norm.weight, norm.bias, norm.eps, y_qfrag=y_qfrag)


# The tail of a SpatialTransformer as one pass (csrc/sta_rowstail.hip): ff.net[2] + the last block's residual, then proj_out + the
# transformer's residual, are one GEMM over [h | x2] against [Wp W2 | Wp]. False: the feed-forward output pass, then proj_out as a row GEMM.
FF_TAIL_PROJ_OUT_C320 = True    # level 0 (C = 320, h in fragment order)
FF_TAIL_PROJ_OUT_C640 = True    # level 1 (C = 640, h row-major)
FF_TAIL_PASS_ROWS = {320: 256, 640: 128}    # rows of one workgroup pass: what rows-per-image must be a multiple of for the statistics


def ff_tail_weights(net2, proj_out):
    """(W', b') of out = x_in + [h | x2] [W' | Wp]^T + b' for x3 = x2 + net2(h), out = x_in + proj_out(x3): W' = Wp W2 ([C, inner]) and
    b' = Wp b2 + bp ([C], None when neither module has a bias). `proj_out`: an nn.Linear or a 1x1 nn.Conv2d. 16-bit weights are
    multiplied in fp32 and W' is rounded ONCE to their dtype; wider types keep their own precision. b' stays in the precision of the
    products (fp32 for 16-bit weights: the kernel reads it as such). Runs on any device."""
    w2, wp = net2.weight.detach(), proj_out.weight.detach()
    wp = wp.reshape(wp.shape[0], wp.shape[1])
    acc = torch.float32 if w2.dtype in (torch.float16, torch.bfloat16) else w2.dtype
    wpa = wp.to(acc)
    w = (wpa @ w2.to(acc)).to(w2.dtype)
    b = None
    if net2.bias is not None:
        b = wpa @ net2.bias.detach().to(acc)
    if proj_out.bias is not None:
        b = proj_out.bias.detach().to(acc) if b is None else b + proj_out.bias.detach().to(acc)
    return w, b


def _is_pointwise(m, C):
    """`m` is a plain nn.Linear [C <- C] or a plain 1x1 nn.Conv2d of C channels (stride 1, no padding, no groups)."""
    if type(m) is torch.nn.Linear:
        return m.in_features == C and m.out_features == C
    return (type(m) is torch.nn.Conv2d and m.in_channels == C and m.out_channels == C and m.kernel_size == (1, 1) and m.stride == (1, 1)
            and m.padding == (0, 0) and m.groups == 1)


def ff_tail_supported(x, net2, proj_out):
    """The switch of x's width is on, `net2` is a plain nn.Linear [C <- 4 C] and `proj_out` a plain nn.Linear / 1x1 nn.Conv2d of C channels, both
    of x's dtype on its device; x [.., C] has a multiple of 16 rows, enough of them for a persistent pass (rowgemm_worthwhile), and the
    [rows, 4 C] input stays below what a launch addresses."""
    C = x.shape[-1]
    if not {320: FF_TAIL_PROJ_OUT_C320, 640: FF_TAIL_PROJ_OUT_C640}.get(C, False):
        return False
    return (type(net2) is torch.nn.Linear and net2.out_features == C and _is_pointwise(proj_out, C)
            and net2.weight.dtype == x.dtype and proj_out.weight.dtype == x.dtype and net2.weight.is_cuda and proj_out.weight.is_cuda
            and (x.numel() // C) % 16 == 0 and rowgemm_worthwhile(x, net2.in_features)
            and bool(lib.load().sta_ff_tail_packed_w_bytes(C, net2.in_features)))


def pack_ff_tail_weight(wcat):
    """[W' | Wp] [C, inner + C] -> the fragment image sta_ff_tail streams through LDS (uint8 tensor); once per model."""
    C, K = wcat.shape
    return _pack_ff_weight(wcat, C, K - C, "sta_ff_tail_packed_w_bytes", "sta_ff_tail_pack_w",
                           "feed-forward output + proj_out: a CUDA weight [320, 1600] or [640, 3200]")


def ff_tail_image(owner, net2, proj_out):
    """(packed [W' | Wp], b' in fp32 or None) of ff_tail_weights(net2, proj_out), cached on `owner` and rebuilt when any of the (up to)
    four tensors changes."""
    tensors = tuple(t for t in (net2.weight, net2.bias, proj_out.weight, proj_out.bias) if t is not None)

    def build():
        w, b = ff_tail_weights(net2, proj_out)
        wp = proj_out.weight.detach()
        return pack_ff_tail_weight(torch.cat([w, wp.reshape(wp.shape[0], wp.shape[1])], dim=1)), (None if b is None else b.float().contiguous())
    return cached_image(owner, ("ff_tail", id(net2), id(proj_out)), tensors, build)


def ff_tail(h, x2, x_in, w_packed, bias=None, stats_rows=None, max_workgroups=0):
    """x_in + [h | x2] [W' | Wp]^T + b' over x2, x_in [.., C] and h [.., 4 C] (row-major at C = 640; at C = 320 in the fragment order of
    ff_geglu_qfrag(h_frag=True)); `w_packed`, `bias` (fp32): ff_tail_image's. One pass (csrc/sta_rowstail.hip). stats_rows = rows per
    image (a multiple of FF_TAIL_PASS_ROWS[C] that divides the rows, refused otherwise): per-image, per-channel sum / sum of squares ride
    on the result as `_sta_stats`, as from linear_rows. `max_workgroups` > 0 caps the grid (tests)."""
    C, inner = x2.shape[-1], h.shape[-1]
    R = x2.numel() // C
    if h.numel() // inner != R or x_in.numel() != x2.numel() or h.dtype != x2.dtype or x_in.dtype != x2.dtype:
        raise ValueError("ff_tail: h %s, x2 %s and x_in %s must have the same rows and dtype" % (tuple(h.shape), tuple(x2.shape), tuple(x_in.shape)))
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != C):
        raise ValueError("ff_tail: b' must be %d fp32 values" % C)
    h, x2, x_in = h.contiguous(), x2.contiguous(), x_in.contiguous()
    out = torch.empty_like(x2)
    part, n_img, slots = None, 0, 0
    if stats_rows:
        n_img, slots = R // stats_rows, max(1, stats_rows // 32)
        part = torch.empty((n_img + 1, slots, C, 2), dtype=torch.float32, device=x2.device)
    lib.check(lib.load().sta_ff_tail(h.data_ptr(), x2.data_ptr(), w_packed.data_ptr(), _ptr(bias), x_in.data_ptr(), out.data_ptr(), _ptr(part),
                                     int(stats_rows or 0), R, C, inner, int(max_workgroups), _DT[x2.dtype], _stream()), "sta_ff_tail")
    if part is not None and _version(out) is not None:
        out._sta_stats = (out._version, _finalize_stats(part, n_img, slots, C))
    return out


class FfTail:
    """What SpatialTransformer hands its LAST block so that the block's feed-forward output pass also applies proj_out and the
    transformer's residual: the module that owns the packed-weight cache, proj_out, the row view of the transformer's input and the
    rows per image (None: no statistics wanted). The block sets `done` when its result IS the transformer's output."""

    def __init__(self, owner, proj_out, x_in, stats_rows):
        self.owner, self.proj_out, self.x_in, self.stats_rows, self.done = owner, proj_out, x_in, stats_rows, False

    def run(self, x2, h, net2):
        """The fused tail over the block's residual stream x2 and GEGLU output h (ff_tail_supported accepted them)."""
        wp, b = ff_tail_image(self.owner, net2, self.proj_out)
        C = x2.shape[-1]
        sr = self.stats_rows if self.stats_rows and self.stats_rows % FF_TAIL_PASS_ROWS[C] == 0 and (x2.numel() // C) % self.stats_rows == 0 else None
        out = ff_tail(h, x2, self.x_in, wp, b, stats_rows=sr)
        self.done = True
        return out


LN_QKV = True           # level 0: norm1 + the q|k and V^T projections of attn1 as one pass (csrc/sta_lnqkv.hip); False: sta_add_layernorm + two library GEMMs


def ln_qkv_supported(x):
    """Shapes sta_ln_qkv takes: C = 320, a multiple of 16 rows, the [rows, 2C] q|k output addressable by one launch."""
    C = x.shape[-1]
    return (x.numel() // C) % 16 == 0 and rows_addressable(x, width=2 * C) and bool(lib.load().sta_ln_qkv_packed_w_bytes(C))


def pack_ln_qkv_weight(wqk, wv):
    """[Wq * scale * log2 e; Wk] [2C, C] and Wv [C, C] -> the fragment image sta_ln_qkv streams through LDS (uint8 tensor); once per model."""
    C = wv.shape[0]
    L = lib.load()
    n = L.sta_ln_qkv_packed_w_bytes(C)
    if n == 0 or tuple(wqk.shape) != (2 * C, C) or tuple(wv.shape) != (C, C) or not wv.is_cuda or wqk.dtype != wv.dtype:
        raise ValueError("fused norm1 + q/k/v projection: CUDA weights [640, 320] and [320, 320] of one dtype; got %s %s" % (tuple(wqk.shape), tuple(wv.shape)))
    wqk, wv = wqk.detach().contiguous(), wv.detach().contiguous()
    buf = torch.empty(n, dtype=torch.uint8, device=wv.device)
    lib.check(L.sta_ln_qkv_pack_w(wqk.data_ptr(), wv.data_ptr(), buf.data_ptr(), C, _DT[wv.dtype], _stream()), "sta_ln_qkv_pack_w")
    return buf


def ln_qkv(x, bias, ln_weight, ln_bias, eps, w_packed, store_sum=True, y_dbg=None):
    """s = x + bias; y = LayerNorm(s); returns (s, qk, vt): qk [.., 2C] = y [Wq'; Wk]^T row-major, vt [C, rows] = Wv y^T — what
    sta.ops.self_attention reads as qk[..., :C], qk[..., C:], vt.view(C, B, N).permute(1, 0, 2). y never reaches HBM unless a test
    hands in `y_dbg` (a tensor like x), which then receives it row-major, bit-identical to add_layernorm's. s is None if store_sum is False."""
    C = x.shape[-1]
    R = x.numel() // C
    x = x.contiguous()
    s = torch.empty_like(x) if store_sum else None
    qk = torch.empty(*x.shape[:-1], 2 * C, dtype=x.dtype, device=x.device)
    vt = torch.empty((C, R), dtype=x.dtype, device=x.device)
    lib.check(lib.load().sta_ln_qkv(x.data_ptr(), _ptr(bias), ln_weight.data_ptr(), ln_bias.data_ptr(), w_packed.data_ptr(), _ptr(s), _ptr(y_dbg),
                                    qk.data_ptr(), vt.data_ptr(), R, C, float(eps), _DT[x.dtype], _stream()), "sta_ln_qkv")
    return s, qk, vt


GN_STATS_FROM_PRODUCER = True   # convolutions / row GEMMs accumulate the consumer GroupNorm's statistics in their epilogue (no statistics pass)
CONV_MIN_ITEMS = 64     # (tile, channel part) work items below which the library convolution is the faster one (a launch feeds 256 CUs:
                        # at one prompt per step the 16 x 16 / 8 x 8 levels have 16 items and lose 2 - 3 x: tools/conv_bench.py --batch 2)
CONV3X3 = True          # the HIP implicit-GEMM 3x3 convolution for the NHWC trunk (csrc/sta_conv.hip); False: library convolution
CONV_UP2_SUBPIXEL = True    # Upsample.conv (`up2`) as four 2x2 sub-pixel convolutions of the half-resolution tensor (4/9 of the flops:
                            # csrc/sta_conv.hip, SUB); False: the 3x3 kernel reading the small tensor through (y >> 1, x >> 1)
_conv_zeros = {}
CONV_MAX_BYTES = 0xfffffff0 - 1     # output bytes one launch addresses (32-bit buffer descriptor)


def _finalize_stats(part, B, slots, C):
    """[B + 1, slots, C, 2] partial sums of a convolution / row GEMM epilogue -> [B, C, 2] (fixed order, no atomics)."""
    st = torch.empty((B, C, 2), dtype=torch.float32, device=part.device)
    lib.check(lib.load().sta_stats_finalize(part.data_ptr(), st.data_ptr(), B, slots, C, _stream()), "sta_stats_finalize")
    return st


def conv3x3_supported(x, weight, up2=False):
    """The HIP 3x3 convolution applies to NHWC 16-bit CUDA activations outside autograd at the geometries
    sta_conv3x3_nhwc_supported lists (the UNet's ResBlock / Upsample convolutions at 512^2 down to the 16x16 level, the VAE
    decoder's 128 / 256 / 512-channel convolutions); one image must stay below the 4 GiB a launch addresses."""
    if not (CONV3X3 and usable(x) and x.dim() == 4 and is_nhwc(x) and weight.dtype == x.dtype and tuple(weight.shape[2:]) == (3, 3)):
        return False
    B, Cin, H, W = x.shape
    if up2:
        H, W = 2 * H, 2 * W
    return bool(lib.load().sta_conv3x3_nhwc_supported(1, H, W, Cin, weight.shape[0])) and conv3x3_work_items(B, H, W, weight.shape[0]) >= CONV_MIN_ITEMS


def conv3x3_work_items(B, H, W, Cout):
    """(pixel tile, output-channel part) items of one sta_conv3x3_nhwc launch: what its 256 persistent workgroups share."""
    slots = lib.load().sta_conv3x3_stats_slots(H, W)
    tiles = (B + 1) // 2 if (H, W) == (8, 8) else B * slots // 4
    return tiles * (Cout // 160 if Cout % 160 == 0 else Cout // 128)


def conv3x3_up2_subpixel_supported(x, weight):
    """x ([B, Cin, Hs, Ws], what conv3x3_supported(x, weight, up2=True) accepted) at a geometry the sub-pixel mode takes (the tiles are
    those of the Hs x Ws input: a 16-wide, 8-high input has none and stays with the 3x3 kernel), with enough (tile, part, phase) items."""
    B, Cin, Hs, Ws = x.shape
    Cout = weight.shape[0]
    return (bool(lib.load().sta_conv3x3_up2_nhwc_supported(1, 2 * Hs, 2 * Ws, Cin, Cout))
            and conv3x3_up2_work_items(B, 2 * Hs, 2 * Ws, Cout) >= CONV_MIN_ITEMS)


def conv3x3_up2_work_items(B, H, W, Cout):
    """(pixel tile of the H / 2 x W / 2 input, output-channel part, output phase) items of one sta_conv3x3_up2_nhwc launch."""
    return 4 * conv3x3_work_items(B, H // 2, W // 2, Cout)


def subpixel_weights(weight):
    """Conv2d weight [Cout, Cin, 3, 3] -> [4, Cout, Cin, 2, 2]: the 2x2 taps W'_ab[u][v] of output phase 2a + b (row, column parity) of
    conv2d(interpolate(x, 2, 'nearest'), weight, padding=1) as a convolution of x itself,
        out[2y + a][2x + b] = sum_{u, v} W'_ab[u][v] . x[y + u + a - 1][x + v + b - 1],
        W'_ab[u][v] = sum_{ky in R_a(u)} sum_{kx in R_b(v)} w[ky][kx],   R_0 = ({0}, {1, 2}),  R_1 = ({0, 1}, {2}).
    The restatement of sta_conv3x3_up2_pack_w: 16-bit weights are summed in fp32, ky-major and kx-minor, and rounded once (wider
    types are summed in their own precision: the unrounded sums). Runs on any device."""
    w = weight.detach()
    acc_dt = torch.float32 if w.dtype in (torch.float16, torch.bfloat16) else w.dtype
    R = (((0,), (1, 2)), ((0, 1), (2,)))
    out = torch.empty((4,) + tuple(w.shape[:2]) + (2, 2), dtype=w.dtype, device=w.device)
    for a in range(2):
        for b in range(2):
            for u in range(2):
                for v in range(2):
                    s = torch.zeros(w.shape[:2], dtype=acc_dt, device=w.device)
                    for ky in R[a][u]:
                        for kx in R[b][v]:
                            s = s + w[:, :, ky, kx].to(acc_dt)
                    out[2 * a + b, :, :, u, v] = s.to(w.dtype)
    return out


def subpixel_conv_reference(x, wsub):
    """The four 2x2 convolutions of the zero-padded x [B, Cin, Hs, Ws] with wsub = subpixel_weights(w) ([4, Cout, Cin, 2, 2]), interleaved
    into [B, Cout, 2 Hs, 2 Ws]: what sta_conv3x3_up2_nhwc computes, in torch and in x's precision (the tests' reference)."""
    B, _, Hs, Ws = x.shape
    xp = torch.nn.functional.pad(x, (1, 1, 1, 1))
    out = x.new_empty((B, wsub.shape[1], 2 * Hs, 2 * Ws))
    for a in range(2):
        for b in range(2):
            out[:, :, a::2, b::2] = torch.nn.functional.conv2d(xp[:, :, a:a + Hs + 1, b:b + Ws + 1], wsub[2 * a + b].to(x.dtype))
    return out


def pack_conv3x3_up2_weight(weight):
    """Conv2d weight [Cout, Cin, 3, 3] (any memory format) -> the A-operand fragment image of sta_conv3x3_up2_nhwc: subpixel_weights(weight)
    as 1-KiB fragments [phase][part][channel step][u][v][tile] (include/sta_unet.h); once per model."""
    Cout, Cin = weight.shape[0], weight.shape[1]
    L = lib.load()
    n = L.sta_conv3x3_up2_packed_w_bytes(Cin, Cout)
    if n == 0 or not weight.is_cuda or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError("conv3x3_up2: a CUDA weight [Cout %% 160 == 0 or Cout %% 128 == 0, Cin %% 64 == 0, 3, 3]; got %s" % (tuple(weight.shape),))
    w = weight.detach()
    buf = torch.empty(n, dtype=torch.uint8, device=w.device)
    so, si, sy, sx = w.stride()
    lib.check(L.sta_conv3x3_up2_pack_w(w.data_ptr(), so, si, sy, sx, buf.data_ptr(), Cin, Cout, _DT[w.dtype], _stream()), "sta_conv3x3_up2_pack_w")
    return buf


def pack_conv3x3_weight(weight):
    """Conv2d weight [Cout, Cin, 3, 3] (any memory format) -> the A-operand fragment image of sta_conv3x3_nhwc; once per model."""
    Cout, Cin = weight.shape[0], weight.shape[1]
    L = lib.load()
    n = L.sta_conv3x3_packed_w_bytes(Cin, Cout)
    if n == 0 or not weight.is_cuda or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError("conv3x3: a CUDA weight [Cout %% 160 == 0 or Cout %% 128 == 0, Cin %% 64 == 0, 3, 3]; got %s" % (tuple(weight.shape),))
    w = weight.detach()
    buf = torch.empty(n, dtype=torch.uint8, device=w.device)
    so, si, sy, sx = w.stride()
    lib.check(L.sta_conv3x3_pack_w(w.data_ptr(), so, si, sy, sx, buf.data_ptr(), Cin, Cout, _DT[w.dtype], _stream()), "sta_conv3x3_pack_w")
    return buf


def conv3x3_nhwc(x, w_packed, Cout, up2=False, bias=None, res=None, stats=False, subpixel=False):
    """conv2d(x, w, bias, padding=1) + res on an NHWC activation (logical shape [B, Cin, H, W], channels_last strides);
    up2: of the nearest-neighbour 2x upsampling of x, which is never written. Returns [B, Cout, H', W'] channels_last.
    A launch addresses its output through one 32-bit buffer descriptor: batches whose output exceeds 4 GiB go in several launches.
    stats: the kernel also accumulates every output channel's sum / sum of squares; they ride on the result as `_sta_stats`
    ([B, Cout, 2] fp32) for the GroupNorm that consumes it (groupnorm_silu skips its statistics pass).
    subpixel (with up2): w_packed is pack_conv3x3_up2_weight's image and the launch is sta_conv3x3_up2_nhwc — the same operation as four
    2x2 convolutions of x, equal to the 3x3 path up to one rounding of every pre-summed weight."""
    assert up2 or not subpixel, "subpixel is a mode of up2"
    B, Cin, Hs, Ws = x.shape
    H, W = (2 * Hs, 2 * Ws) if up2 else (Hs, Ws)
    z = _zeros_page(x.device, 2 * Cin)
    out = torch.empty((B, Cout, H, W), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    if res is not None:
        assert res.shape == out.shape and res.dtype == x.dtype and (is_nhwc(res) or res.is_contiguous(memory_format=torch.channels_last))
    if bias is not None:
        bias = bias.to(x.dtype).contiguous()
    esz = x.element_size()
    per_img = H * W * Cout * esz
    nb = max(1, min(B, CONV_MAX_BYTES // per_img))
    L = lib.load()
    slots = (L.sta_conv3x3_up2_stats_slots(H, W) if subpixel else L.sta_conv3x3_stats_slots(H, W)) if stats else 0
    part = torch.empty((B + 1, slots, Cout, 2), dtype=torch.float32, device=x.device) if slots else None
    for b0 in range(0, B, nb):
        n = min(nb, B - b0)
        # (a chunk's spare image slot is the next chunk's first image, written later; the last chunk's is the tensor's spare slot)
        ptrs = (x.data_ptr() + b0 * Hs * Ws * Cin * esz, w_packed.data_ptr(), z.data_ptr(), _ptr(bias),
                0 if res is None else res.data_ptr() + b0 * per_img, out.data_ptr() + b0 * per_img,
                0 if part is None else part.data_ptr() + b0 * slots * Cout * 8)
        if subpixel:
            lib.check(L.sta_conv3x3_up2_nhwc(*ptrs, n, H, W, Cin, Cout, _DT[x.dtype], _stream()), "sta_conv3x3_up2_nhwc")
        else:
            lib.check(L.sta_conv3x3_nhwc(*ptrs, n, H, W, Cin, Cout, int(bool(up2)), _DT[x.dtype], _stream()), "sta_conv3x3_nhwc")
    if part is not None:
        if _version(out) is not None:           # (inference tensors: no producer statistics, the consumer takes its own pass)
            out._sta_stats = (out._version, _finalize_stats(part, B, slots, Cout))
    return out


def packed_conv_weight(owner, conv):
    """conv.weight as sta_conv3x3_nhwc streams it, cached on the owning module and repacked only when the weight tensor changes."""
    w = conv.weight
    return cached_image(owner, ("conv", id(conv)), (w,), lambda: pack_conv3x3_weight(w))


def packed_conv_up2_weight(owner, conv):
    """conv.weight as sta_conv3x3_up2_nhwc streams it (the sub-pixel image), cached under a slot of its own and repacked as above."""
    w = conv.weight
    return cached_image(owner, ("conv_up2", id(conv)), (w,), lambda: pack_conv3x3_up2_weight(w))


def conv3x3_module(owner, conv, x, bias=None, res=None, up2=False, stats=True):
    """conv(x) (+ bias + res) for a 3x3 nn.Conv2d outside autograd: the HIP convolution where it applies, the library convolution
    (+ the fused bias / residual pass) elsewhere. `bias=None` means bias-free (the caller folds conv.bias into a later pass).
    `stats=False`: the result is not read by a GroupNorm next (e.g. it feeds an Upsample convolution) — no epilogue statistics, no
    partial buffer, no finalize launch."""
    if conv3x3_supported(x, conv.weight, up2=up2) and (res is None or is_nhwc(res)):
        if up2 and CONV_UP2_SUBPIXEL and conv3x3_up2_subpixel_supported(x, conv.weight):
            return conv3x3_nhwc(x, packed_conv_up2_weight(owner, conv), conv.weight.shape[0], up2=True, bias=bias, res=res,
                                stats=GN_STATS_FROM_PRODUCER and stats, subpixel=True)
        return conv3x3_nhwc(x, packed_conv_weight(owner, conv), conv.weight.shape[0], up2=up2, bias=bias, res=res,
                            stats=GN_STATS_FROM_PRODUCER and stats)
    if up2:
        x = torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")
    h = torch.nn.functional.conv2d(x, conv.weight, None, conv.stride, conv.padding)
    return h if bias is None and res is None else add_bias_nchw(h if res is None else res, None if res is None else h, bias)


CONV_S2 = True          # the HIP stride-2 3x3 convolution of the VAE encoder's Downsample (csrc/sta_encode.hip); False: F.pad + library
CONV_S2_MIN_ITEMS = 64  # (8 x 16 output tile, 128-channel part) work items below which F.pad + the library convolution stays


def conv3x3_s2_work_items(B, H, W, Cout):
    """Workgroups of one sta_conv3x3_s2_nhwc launch over an H x W input (8 x 16 output tiles x 128-channel parts)."""
    return B * (H // 16) * (W // 32) * (Cout // 128)


def conv3x3_s2_supported(x, weight):
    """The HIP Downsample convolution (pad (0, 1, 0, 1), 3x3, stride 2) applies to NHWC 16-bit CUDA activations outside autograd at the
    geometries sta_conv3x3_s2_nhwc_supported lists (one image below the 4 GiB a launch addresses)."""
    if not (CONV_S2 and usable(x) and x.dim() == 4 and is_nhwc(x) and weight.dtype == x.dtype and tuple(weight.shape[2:]) == (3, 3)):
        return False
    B, Cin, H, W = x.shape
    Cout = weight.shape[0]
    return bool(lib.load().sta_conv3x3_s2_nhwc_supported(1, H, W, Cin, Cout)) and conv3x3_s2_work_items(B, H, W, Cout) >= CONV_S2_MIN_ITEMS


def conv3x3_s2_nhwc(x, w_packed, Cout, bias=None, stats=False):
    """conv2d(F.pad(x, (0, 1, 0, 1)), w, bias, stride=2) on an NHWC activation [B, Cin, H, W] (channels_last strides); the padded tensor is
    never written. w_packed: pack_conv3x3_weight's image. Returns [B, Cout, H / 2, W / 2] channels_last; `stats` as for conv3x3_nhwc."""
    B, Cin, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    z = _zeros_page(x.device, 2 * Cin)
    out = torch.empty((B, Cout, Ho, Wo), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    if bias is not None:
        bias = bias.to(x.dtype).contiguous()
    esz = x.element_size()
    per_in, per_out = H * W * Cin * esz, Ho * Wo * Cout * esz
    nb = max(1, min(B, CONV_MAX_BYTES // per_in))
    L = lib.load()
    slots = L.sta_conv3x3_s2_stats_slots(H, W) if stats else 0
    part = torch.empty((B + 1, slots, Cout, 2), dtype=torch.float32, device=x.device) if slots else None
    for b0 in range(0, B, nb):
        n = min(nb, B - b0)
        lib.check(L.sta_conv3x3_s2_nhwc(x.data_ptr() + b0 * per_in, w_packed.data_ptr(), z.data_ptr(), _ptr(bias), out.data_ptr() + b0 * per_out,
                                        0 if part is None else part.data_ptr() + b0 * slots * Cout * 8, n, H, W, Cin, Cout, _DT[x.dtype],
                                        _stream()), "sta_conv3x3_s2_nhwc")
    if part is not None and _version(out) is not None:
        out._sta_stats = (out._version, _finalize_stats(part, B, slots, Cout))
    return out


def vae_encode_step(h, quant_weight, quant_bias, n_post, n_enc, scale_factor, sqrt_a, sqrt_1ma, want_z0=False, want_xin=True):
    """The encoder's conv_out result h [B, 8, h, w] (16-bit CUDA, channels_last) -> (x, z0, xin) in one pass (sta_vae_encode_step):
    quant_conv, the posterior's sample z0 = scale_factor (mean + std n_post), x = sqrt_a z0 + sqrt_1ma n_enc (fp32 [B, 4, h, w]), xin the
    16-bit CFG input pair [2B, 4, h, w] of x. n_post, n_enc: fp32 [B, 4, h, w] noises."""
    B, C, Hh, Ww = h.shape
    if C != 8 or not h.is_cuda or h.dtype not in _DT:
        raise ValueError("vae_encode_step: 16-bit CUDA h [B, 8, h, w], got %s %s" % (tuple(h.shape), h.dtype))
    h = h.contiguous(memory_format=torch.channels_last)
    qw = quant_weight.detach().reshape(8, 8).float().contiguous()
    qb = quant_bias.detach().float().contiguous()
    f = lambda t: t.detach().to(device=h.device, dtype=torch.float32).contiguous()
    n_post, n_enc = f(n_post), f(n_enc)
    if n_post.shape != (B, 4, Hh, Ww) or n_enc.shape != (B, 4, Hh, Ww):
        raise ValueError("vae_encode_step: noises must be [B, 4, h, w] = %s" % ((B, 4, Hh, Ww),))
    x = torch.empty((B, 4, Hh, Ww), dtype=torch.float32, device=h.device)
    z0 = torch.empty_like(x) if want_z0 else None
    xin = torch.empty((2 * B, 4, Hh, Ww), dtype=h.dtype, device=h.device) if want_xin else None
    lib.check(lib.load().sta_vae_encode_step(h.data_ptr(), qw.data_ptr(), qb.data_ptr(), n_post.data_ptr(), n_enc.data_ptr(), x.data_ptr(),
                                             _ptr(z0), _ptr(xin), B, Hh * Ww, float(scale_factor), float(sqrt_a), float(sqrt_1ma), _DT[h.dtype],
                                             _stream()), "sta_vae_encode_step")
    return x, z0, xin


CAT_IN_PLACE = True     # output blocks read `cat([h, skip])` in place (GroupNorm and the 1x1 skip GEMM take both tensors); False: torch.cat


def groupnorm_silu_cat(xa, xb, weight, bias, groups, eps, silu=True):
    """act(GroupNorm(cat([xa, xb], dim=1))) for two NHWC activations, the concatenation read in place (csrc/sta_unet.hip);
    returns the normalised concatenated tensor. Callers check cat_supported first."""
    B, Ca = xa.shape[0], xa.shape[1]
    C = Ca + xb.shape[1]
    HW = xa.numel() // (B * Ca)
    L = lib.load()
    y = torch.empty((B, C) + tuple(xa.shape[2:]), dtype=xa.dtype, device=xa.device, memory_format=torch.channels_last)
    sa, sb = (_producer_stats(xa), _producer_stats(xb)) if GN_STATS_FROM_PRODUCER else (None, None)
    if sa is not None and sb is not None:
        lib.check(L.sta_groupnorm_silu_nhwc_cstats(xa.data_ptr(), xb.data_ptr(), Ca, sa.data_ptr(), sb.data_ptr(), None, weight.data_ptr(),
                                                   bias.data_ptr(), y.data_ptr(), B, C, HW, groups, float(eps), int(bool(silu)), _DT[xa.dtype],
                                                   _stream()), "sta_groupnorm_silu_nhwc_cstats")
        return y
    ws = torch.empty(L.sta_groupnorm_nhwc_workspace_bytes(B, HW, groups) // 4, dtype=torch.float32, device=xa.device)
    lib.check(L.sta_groupnorm_silu_nhwc_cat(xa.data_ptr(), xb.data_ptr(), Ca, None, weight.data_ptr(), bias.data_ptr(), y.data_ptr(),
                                            ws.data_ptr(), B, C, HW, groups, float(eps), int(bool(silu)), _DT[xa.dtype], _stream()),
              "sta_groupnorm_silu_nhwc_cat")
    return y


def cat_supported(xa, xb, groups, skip_weight):
    """Both halves NHWC 16-bit outside autograd, channel counts the in-place GroupNorm and the in-place 1x1 skip GEMM take."""
    if not (CAT_IN_PLACE and usable(xa) and is_nhwc(xa) and is_nhwc(xb) and xa.dtype == xb.dtype and xa.shape[0] == xb.shape[0]
            and xa.shape[2:] == xb.shape[2:]):
        return False
    Ca, C = xa.shape[1], xa.shape[1] + xb.shape[1]
    if Ca % 64 or C % 8 or C % groups or (C // groups < 8 and C // groups != 4) or C > 4096 or groups > 64:
        return False
    rows = xa.numel() // Ca
    return (LINEAR_ROWS and rows >= LINEAR_MIN_ROWS and skip_weight.dtype == xa.dtype
            and bool(lib.load().sta_linear_rows_supported(rows, C, skip_weight.shape[0])))


def linear_rows_cat(xa, xb, w_packed, N, bias=None, res=None):
    """cat([xa, xb], dim=-1) @ W^T + bias + res over row tensors [..., Ka] and [..., Kb], the concatenation read in place."""
    Ka, Kb = xa.shape[-1], xb.shape[-1]
    R = xa.numel() // Ka
    assert xa.is_contiguous() and xb.is_contiguous() and xb.numel() // Kb == R and Ka % 64 == 0
    out = torch.empty(xa.shape[:-1] + (N,), dtype=xa.dtype, device=xa.device)
    if bias is not None:
        bias = bias.to(xa.dtype).contiguous()
    z = _zeros_page(xa.device, 2 * (Ka + Kb))
    lib.check(lib.load().sta_linear_rows_cat(xa.data_ptr(), xb.data_ptr(), Ka, w_packed.data_ptr(), z.data_ptr(), _ptr(bias), _ptr(res),
                                             out.data_ptr(), R, Ka + Kb, N, _DT[xa.dtype], _stream()), "sta_linear_rows_cat")
    return out


LINEAR_ROWS = True      # the HIP row GEMM for Linear layers / 1x1 convolutions outside autograd (csrc/sta_gemm.hip); False: library GEMM
LINEAR_MIN_ROWS = 4096  # below this many rows the library GEMM stays (time-embedding, context projections)


_retired_pages = []


def _zeros_page(device, nbytes):
    """The page of zeros the convolution / row GEMM kernels read their padding from. Captured hipGraphs hold its address: a page
    that had to grow is kept alive, never freed."""
    z = _conv_zeros.get(device)
    if z is None or z.numel() < nbytes:
        if z is not None:
            _retired_pages.append(z)
        z = _conv_zeros[device] = torch.zeros(max(nbytes, 16384), dtype=torch.uint8, device=device)
    return z


def linear_rows_supported(x, weight):
    """The HIP row GEMM applies to dense 16-bit CUDA rows outside autograd: x [..., K] contiguous, weight [N, K] (or [N, K, 1, 1])
    with K % 64 == 0 and N % 160 == 0 or N % 128 == 0, at least LINEAR_MIN_ROWS rows, output below 4 GiB."""
    if not (LINEAR_ROWS and x.is_cuda and x.dtype in _DT and not torch.is_grad_enabled() and ENABLED and not _hold and weight.dtype == x.dtype):
        return False
    K = x.shape[-1]
    R = x.numel() // K
    return R >= LINEAR_MIN_ROWS and x.is_contiguous() and bool(lib.load().sta_linear_rows_supported(R, K, weight.shape[0]))


def pack_linear_weight(weight):
    """Linear weight [N, K] (or a 1x1 Conv2d weight [N, K, 1, 1], any memory format) -> the A-operand fragment image of sta_linear_rows."""
    N, K = weight.shape[0], weight.shape[1]
    L = lib.load()
    n = L.sta_linear_rows_packed_w_bytes(K, N)
    if n == 0 or not weight.is_cuda:
        raise ValueError("linear_rows: a CUDA weight [N %% 160 == 0 or N %% 128 == 0, K %% 64 == 0]; got %s" % (tuple(weight.shape),))
    w = weight.detach()
    buf = torch.empty(n, dtype=torch.uint8, device=w.device)
    lib.check(L.sta_linear_rows_pack_w(w.data_ptr(), w.stride(0), w.stride(1), buf.data_ptr(), K, N, _DT[w.dtype], _stream()), "sta_linear_rows_pack_w")
    return buf


def linear_rows(x, w_packed, N, bias=None, res=None, stats_rows=None):
    """x @ W^T + bias + res over the rows of a contiguous [..., K] tensor; returns [..., N] (csrc/sta_gemm.hip).
    stats_rows = rows per image (a multiple of 256): per-image, per-column sum / sum of squares ride on the result as `_sta_stats`."""
    K = x.shape[-1]
    R = x.numel() // K
    out = torch.empty(x.shape[:-1] + (N,), dtype=x.dtype, device=x.device)
    if res is not None:
        assert res.numel() == out.numel() and res.dtype == x.dtype and res.is_contiguous()
    if bias is not None:
        bias = bias.to(x.dtype).contiguous()
    z = _zeros_page(x.device, 2 * K)
    if stats_rows and stats_rows % 256 == 0 and R % stats_rows == 0:
        n_img, slots = R // stats_rows, stats_rows // 64
        part = torch.empty((n_img + 1, slots, N, 2), dtype=torch.float32, device=x.device)
        lib.check(lib.load().sta_linear_rows_stats(x.data_ptr(), w_packed.data_ptr(), z.data_ptr(), _ptr(bias), _ptr(res), out.data_ptr(),
                                                   part.data_ptr(), stats_rows, R, K, N, _DT[x.dtype], _stream()), "sta_linear_rows_stats")
        if _version(out) is not None:
            out._sta_stats = (out._version, _finalize_stats(part, n_img, slots, N))
        return out
    lib.check(lib.load().sta_linear_rows(x.data_ptr(), w_packed.data_ptr(), z.data_ptr(), _ptr(bias), _ptr(res), out.data_ptr(), R, K, N,
                                         _DT[x.dtype], _stream()), "sta_linear_rows")
    return out


def packed_linear_weight(owner, key_obj, weight):
    """weight as sta_linear_rows streams it, cached on the owning module and repacked only when the weight tensor changes."""
    return cached_image(owner, ("linear", id(key_obj)), (weight,), lambda: pack_linear_weight(weight))


def linear_module(lin, x, res=None):
    """lin(x) (+ res) for an nn.Linear outside autograd: the HIP row GEMM where it applies, the library GEMM elsewhere."""
    if linear_rows_supported(x, lin.weight) and (res is None or res.is_contiguous()):
        return linear_rows(x, packed_linear_weight(lin, lin, lin.weight), lin.weight.shape[0], bias=lin.bias, res=res)
    y = torch.nn.functional.linear(x, lin.weight, lin.bias)
    return y if res is None else y + res


def add_bias_nchw(a, b=None, bias=None):
    """a + b + bias[None, :, None, None] over 4-D activations (both NCHW-contiguous or both channels_last)."""
    B, C = a.shape[0], a.shape[1]
    HW = a.numel() // (B * C)
    if (C % 8 if is_nhwc(a) else HW % 8):
        t = a if b is None else a + b
        return t if bias is None else t + bias[None, :, None, None]
    y = torch.empty_like(a)
    if is_nhwc(a):
        if b is not None and not is_nhwc(b):
            b = b.contiguous(memory_format=torch.channels_last)
        lib.check(lib.load().sta_add_bias_rows(a.data_ptr(), _ptr(b), _ptr(bias), y.data_ptr(), B * HW, C, _DT[a.dtype], _stream()),
                  "sta_add_bias_rows")
        return y
    if b is not None and not b.is_contiguous():
        b = b.contiguous()
    lib.check(lib.load().sta_add_bias_nchw(a.data_ptr(), _ptr(b), _ptr(bias), y.data_ptr(), B, C, HW, _DT[a.dtype], _stream()),
              "sta_add_bias_nchw")
    return y


# -- differentiable forms for the tracked epochs ----------------------------------------------------------------------
def tracked_usable(x):
    """The differentiable fused glue ops apply while autograd records, on dense 16-bit CUDA activations (4-D ones in NHWC)."""
    return (TRACKED and ENABLED and x.is_cuda and x.dtype in _DT and torch.is_grad_enabled()
            and (is_nhwc(x) if x.dim() == 4 else x.is_contiguous()))


class GroupNormSiLUFn(torch.autograd.Function):
    """act(GroupNorm(x + add[:, :, None, None])) on an NHWC activation; backward = sta_groupnorm_silu_nhwc_bwd."""

    @staticmethod
    def forward(ctx, x, add, weight, bias, groups, eps, silu):
        B, C = x.shape[0], x.shape[1]
        HW = x.numel() // (B * C)
        L = lib.load()
        add = None if add is None else add.float().contiguous()
        y = torch.empty_like(x)
        ws = torch.empty(L.sta_groupnorm_nhwc_workspace_bytes(B, HW, groups) // 4, dtype=torch.float32, device=x.device)
        lib.check(L.sta_groupnorm_silu_nhwc(x.data_ptr(), _ptr(add), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                            B, C, HW, groups, float(eps), int(bool(silu)), _DT[x.dtype], _stream()), "sta_groupnorm_silu_nhwc")
        ctx.save_for_backward(x, add, weight, bias, ws)
        ctx.cfg = (B, C, HW, groups, float(eps), int(bool(silu)))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, add, weight, bias, ws = ctx.saved_tensors
        B, C, HW, groups, eps, silu = ctx.cfg
        if not is_nhwc(dy):
            dy = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.empty_like(x)
        wsb = torch.empty_like(ws)
        lib.check(lib.load().sta_groupnorm_silu_nhwc_bwd(x.data_ptr(), _ptr(add), weight.data_ptr(), bias.data_ptr(), dy.data_ptr(),
                                                         dx.data_ptr(), ws.data_ptr(), wsb.data_ptr(), B, C, HW, groups, eps, silu,
                                                         _DT[x.dtype], _stream()), "sta_groupnorm_silu_nhwc_bwd")
        return dx, None, None, None, None, None, None


def groupnorm_silu_tracked(x, weight, bias, groups, eps, add=None, silu=True):
    """Differentiable GroupNorm(+pre-add)(+SiLU) for NHWC activations (eager chain outside the kernel's limits)."""
    C = x.shape[1]
    if add is not None and add.requires_grad:
        raise RuntimeError("the pre-add of the fused GroupNorm carries no gradient (timestep embedding)")
    if not is_nhwc(x) or C % 8 or (C // groups < 8 and C // groups != 4) or C > 4096 or groups > 64:
        h = x if add is None else x + add.to(x.dtype)[:, :, None, None]
        h = torch.nn.functional.group_norm(h, groups, weight, bias, eps)
        return torch.nn.functional.silu(h) if silu else h
    return GroupNormSiLUFn.apply(x, add, weight, bias, groups, eps, silu)


class GegluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h):
        ctx.save_for_backward(h)
        return geglu(h)

    @staticmethod
    def backward(ctx, dy):
        (h,) = ctx.saved_tensors
        D = h.shape[-1] // 2
        dy = dy.contiguous()
        dh = torch.empty_like(h)
        lib.check(lib.load().sta_geglu_bwd(h.data_ptr(), dy.data_ptr(), dh.data_ptr(), h.numel() // (2 * D), D, _DT[h.dtype], _stream()),
                  "sta_geglu_bwd")
        return dh


def geglu_tracked(h):
    if (h.shape[-1] // 2) % 8 or not h.is_contiguous():
        a, gate = h.chunk(2, dim=-1)
        return a * torch.nn.functional.gelu(gate)
    return GegluFn.apply(h)


class AddLayerNormFn(torch.autograd.Function):
    """(s, y) = (x + f + bias, LayerNorm(s)); backward: ds_total = ds + dLayerNorm(dy), handed to x and f alike."""

    @staticmethod
    def forward(ctx, x, f, bias, ln_weight, ln_bias, eps):
        s, y = add_layernorm(x, f, bias, ln_weight, ln_bias, eps, store_sum=True)
        ctx.save_for_backward(s, ln_weight)
        ctx.eps, ctx.has_f = float(eps), f is not None
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        s, ln_weight = ctx.saved_tensors
        C = s.shape[-1]
        dy = dy.contiguous()
        ds = None if ds is None else ds.contiguous()
        g = torch.empty_like(s)
        lib.check(lib.load().sta_layernorm_bwd(s.data_ptr(), ln_weight.data_ptr(), dy.data_ptr(), _ptr(ds), g.data_ptr(), s.numel() // C, C,
                                               ctx.eps, _DT[s.dtype], _stream()), "sta_layernorm_bwd")
        return g, (g if ctx.has_f else None), None, None, None, None


def add_layernorm_tracked(x, f, bias, ln_weight, ln_bias, eps):
    """Differentiable (x + f + bias, LayerNorm(x + f + bias)); x, f [.., C] contiguous."""
    C = x.shape[-1]
    if C % 8 or C > 2048 or not x.is_contiguous() or (f is not None and not f.is_contiguous()):
        t = x if f is None else x + f
        t = t if bias is None else t + bias
        return t, torch.nn.functional.layer_norm(t, (C,), ln_weight, ln_bias, eps)
    return AddLayerNormFn.apply(x, f, bias, ln_weight, ln_bias, eps)


class AddBiasFn(torch.autograd.Function):
    """a + b + bias[None, :, None, None] (NHWC); backward hands dy to a and b."""

    @staticmethod
    def forward(ctx, a, b, bias):
        ctx.has_b = b is not None
        return add_bias_nchw(a, b, bias)

    @staticmethod
    def backward(ctx, dy):
        return dy, (dy if ctx.has_b else None), None


class Conv3x3Fn(torch.autograd.Function):
    """conv2d(x, w, padding=1) without bias on an NHWC activation with FROZEN weights: forward and input gradient are both
    csrc/sta_conv.hip — the input gradient of a 3x3 / stride-1 / padding-1 convolution is the same convolution with the weight's
    channel axes exchanged and its taps mirrored (packed once per model next to the forward image)."""

    @staticmethod
    def forward(ctx, x, wp_fwd, wp_bwd, cin, cout):
        ctx.wp_bwd, ctx.cin = wp_bwd, cin
        return conv3x3_nhwc(x, wp_fwd, cout)

    @staticmethod
    def backward(ctx, dy):
        if not is_nhwc(dy):
            dy = dy.contiguous(memory_format=torch.channels_last)
        return conv3x3_nhwc(dy, ctx.wp_bwd, ctx.cin), None, None, None, None


def conv3x3_tracked_supported(x, weight):
    """The differentiable HIP convolution applies while autograd records (tracked epochs, fused.TRACKED) to NHWC 16-bit activations
    and frozen 3x3 weights whose forward AND mirrored images both fit the kernel's channel rules."""
    if not (CONV3X3 and tracked_usable(x) and x.dim() == 4 and is_nhwc(x) and weight.dtype == x.dtype and not weight.requires_grad
            and tuple(weight.shape[2:]) == (3, 3)):
        return False
    B, Cin, H, W = x.shape
    L = lib.load()
    Cout = weight.shape[0]
    return (bool(L.sta_conv3x3_nhwc_supported(1, H, W, Cin, Cout) and L.sta_conv3x3_nhwc_supported(1, H, W, Cout, Cin))
            and min(conv3x3_work_items(B, H, W, Cout), conv3x3_work_items(B, H, W, Cin)) >= CONV_MIN_ITEMS)


def conv3x3_tracked(owner, conv, x):
    """conv(x) WITHOUT its bias for a frozen 3x3 nn.Conv2d under autograd (callers fold the bias into the pass that follows)."""
    w = conv.weight

    def mirrored():                 # the input gradient's weight: channel axes exchanged, taps mirrored
        with torch.no_grad():
            return pack_conv3x3_weight(w.detach().permute(1, 0, 2, 3).flip(2, 3))
    return Conv3x3Fn.apply(x, packed_conv_weight(owner, conv), cached_image(owner, ("conv_bwd", id(conv)), (w,), mirrored), w.shape[1], w.shape[0])


def add_bias_tracked(a, b=None, bias=None):
    if not is_nhwc(a) or a.shape[1] % 8 or (b is not None and not is_nhwc(b)):
        t = a if b is None else a + b
        return t if bias is None else t + bias[None, :, None, None]
    return AddBiasFn.apply(a, b, bias)
