"""The NHWC GroupNorm (+ pre-add) (+ SiLU) kernels of csrc/sta_unet.hip through their four C entry points, at the smallest shapes at
which the streaming loop (2 or 4 pixels per trip by the pixels a thread has, clamped loads, a predicated last trip) and the 16-lanes-per-group statistics fold
can go wrong. Reference: torch.nn.functional.group_norm (+ silu) in float64 on the same 16-bit inputs; bound: the one
tests/test_fused_gpu.py::test_groupnorm_silu_channels_last applies (3 eps (1 + |ref|)). The per-channel sums the `cstats` entry
point takes are computed in float64 on the host, so no producer kernel is involved."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
GN_EPS = 1e-5


def _close(got, ref, dtype, k=3.0):
    err = (got.float().cpu() - ref).abs()
    tol = k * EPS[dtype] * (1.0 + ref.abs())
    assert (err <= tol).all(), "max err %.4g at tol %.4g" % (err.max().item(), tol.max().item())


# (B, C, G, H, W, Ca): Ca = 0 is one tensor, otherwise the input is the concatenation of Ca and C - Ca channels read in place
PLAIN = [
    (2, 32, 8, 4, 4, 0),         # Cg = 4
    (2, 96, 8, 10, 10, 0),       # a column straddles two groups; ragged last chunk
    (3, 320, 32, 8, 8, 0),       # 8 chunks of 8 px; R = 12 leaves rows idle
    (1, 320, 32, 64, 64, 0),     # the bench's 128-px chunk: 10 or 11 pixels per thread, no multiple of 4 (long-trip variant)
    (2, 2560, 32, 32, 32, 0),    # R = 1, 32 pixels per thread: whole 4-pixel trips only
    (2, 2560, 32, 4, 4, 0),      # Cg = 80 fold; two chunks
    (1, 4096, 32, 2, 4, 0),      # one chunk; CV = 512; Cg = 128
    (2, 512, 64, 8, 8, 0),       # G = 64: two fold rounds
]
CAT = [
    (2, 960, 32, 16, 16, 640),   # concatenation, Ca = 640
    (2, 128, 8, 12, 12, 64),     # concatenation boundary inside a thread row; HW = 144
    (1, 960, 32, 64, 64, 640),   # a concatenation on the long-trip variant of the apply kernel (32 pixels per thread)
]
RAGGED = [PLAIN[0], PLAIN[1], PLAIN[2], PLAIN[3], CAT[1]]
FLAGS = [(True, False), (True, True), (False, False), (False, True)]     # (silu, with_add)
DTYPES = [torch.float16, torch.bfloat16]


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype):
    """Seeded host tensors of a shape: x [B][HW][C] (NHWC), gamma, beta in `dtype`, add [B][C] fp32, and the float64 per-channel
    sums [B][C][2] of x (sum, sum of squares over the pixels) rounded to fp32."""
    B, C, G, H, W, Ca = shape
    g = torch.Generator().manual_seed(B * C + H * W)
    x = (torch.randn(B, H * W, C, generator=g) * 1.7 + 0.3).to(dtype)
    w = (1.0 + 0.2 * torch.randn(C, generator=g)).to(dtype)
    b = (0.2 * torch.randn(C, generator=g)).to(dtype)
    add = torch.randn(B, C, generator=g)
    xd = x.double()
    stats = torch.stack([xd.sum(1), (xd * xd).sum(1)], dim=-1).float()
    return x, w, b, add, stats


@functools.lru_cache(maxsize=None)
def _reference(shape, dtype, silu, with_add):
    B, C, G, H, W, Ca = shape
    x, w, b, add, _ = _inputs(shape, dtype)
    xin = x.double().permute(0, 2, 1)                                   # [B][C][HW]
    if with_add:
        xin = xin + add.double()[:, :, None]
    ref = F.group_norm(xin, G, w.double(), b.double(), GN_EPS)
    ref = F.silu(ref) if silu else ref
    return ref.permute(0, 2, 1).contiguous()                            # [B][HW][C]


@functools.lru_cache(maxsize=None)
def _device(shape, dtype):
    """The inputs on the GPU: the whole x and, for a concatenation, its two halves as tensors of their own."""
    B, C, G, H, W, Ca = shape
    x, w, b, add, stats = _inputs(shape, dtype)
    d = dict(x=x.cuda(), w=w.cuda(), b=b.cuda(), add=add.cuda(), stats=stats.cuda())
    if Ca:
        d.update(xa=x[:, :, :Ca].contiguous().cuda(), xb=x[:, :, Ca:].contiguous().cuda(),
                 stats_a=stats[:, :Ca].contiguous().cuda(), stats_b=stats[:, Ca:].contiguous().cuda())
    return d


def _launch(path, shape, dtype, silu, with_add, y_ptr, ws_ptr=None):
    """One call of entry point `path` ("two", "two_cat", "cstats", "cstats_cat") writing at y_ptr; -> the tensors kept alive."""
    from sta import lib
    L = lib.load()
    B, C, G, H, W, Ca = shape
    HW, dt = H * W, lib.STA_F16 if dtype == torch.float16 else lib.STA_BF16
    d = _device(shape, dtype)
    add = d["add"].data_ptr() if with_add else None
    st = torch.cuda.current_stream().cuda_stream
    keep = None
    if path in ("two", "two_cat") and ws_ptr is None:
        keep = torch.empty(L.sta_groupnorm_nhwc_workspace_bytes(B, HW, G) // 4, dtype=torch.float32, device="cuda")
        ws_ptr = keep.data_ptr()
    if path == "two":
        rc = L.sta_groupnorm_silu_nhwc(d["x"].data_ptr(), add, d["w"].data_ptr(), d["b"].data_ptr(), y_ptr, ws_ptr, B, C, HW, G, GN_EPS,
                                       int(silu), dt, st)
    elif path == "two_cat":
        rc = L.sta_groupnorm_silu_nhwc_cat(d["xa"].data_ptr(), d["xb"].data_ptr(), Ca, add, d["w"].data_ptr(), d["b"].data_ptr(), y_ptr,
                                           ws_ptr, B, C, HW, G, GN_EPS, int(silu), dt, st)
    elif path == "cstats":
        rc = L.sta_groupnorm_silu_nhwc_cstats(d["x"].data_ptr(), None, C, d["stats"].data_ptr(), None, add, d["w"].data_ptr(),
                                              d["b"].data_ptr(), y_ptr, B, C, HW, G, GN_EPS, int(silu), dt, st)
    else:
        rc = L.sta_groupnorm_silu_nhwc_cstats(d["xa"].data_ptr(), d["xb"].data_ptr(), Ca, d["stats_a"].data_ptr(), d["stats_b"].data_ptr(),
                                              add, d["w"].data_ptr(), d["b"].data_ptr(), y_ptr, B, C, HW, G, GN_EPS, int(silu), dt, st)
    lib.check(rc, path)
    return keep


def _run(path, shape, dtype, silu, with_add):
    B, C, G, H, W, Ca = shape
    y = torch.empty(B, H * W, C, dtype=dtype, device="cuda")
    _launch(path, shape, dtype, silu, with_add, y.data_ptr())
    torch.cuda.synchronize()
    return y


def _cases():
    for shape in PLAIN + CAT:
        for path in ("two", "cstats") + (("two_cat", "cstats_cat") if shape[5] else ()):
            yield pytest.param(shape, path, id="%dx%dg%d_%dx%d%s-%s" % (shape[:5] + ("_ca%d" % shape[5] if shape[5] else "", path)))


@pytest.mark.parametrize("silu,with_add", FLAGS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,path", list(_cases()))
def test_gn_stream_against_float64(shape, path, dtype, silu, with_add):
    """Every entry point, both dtypes, silu on / off, with / without the pre-add (a concatenated shape runs the two plain entry points
    on the materialised concatenation as well)."""
    got = _run(path, shape, dtype, silu, with_add)
    ref = _reference(shape, dtype, silu, with_add)
    err = (got.float().cpu() - ref).abs()
    print("max err / (eps (1 + |ref|)) = %.3f" % (err / (EPS[dtype] * (1.0 + ref.abs()))).max().item())
    _close(got, ref, dtype)


@pytest.mark.parametrize("path", ["two", "cstats"])
@pytest.mark.parametrize("shape", RAGGED, ids=lambda s: "%dx%dg%d_%dx%d_ca%d" % s)
def test_gn_stream_writes_nothing_outside_y(shape, path):
    """y (and the two-kernel path's workspace) lie in the middle of sentinel-filled buffers: every byte before and after stays."""
    from sta import lib
    B, C, G, H, W, Ca = shape
    dtype, pad, fill = torch.float16, 1 << 16, 0x5A
    if Ca:
        path += "_cat"
    n = B * H * W * C * 2
    buf = torch.full((pad + n + pad,), fill, dtype=torch.uint8, device="cuda")
    nws = lib.load().sta_groupnorm_nhwc_workspace_bytes(B, H * W, G)
    wsb = torch.full((pad + nws + pad,), fill, dtype=torch.uint8, device="cuda")
    _launch(path, shape, dtype, True, True, buf.data_ptr() + pad, wsb.data_ptr() + pad)
    torch.cuda.synchronize()
    for b, size in ((buf, n), (wsb, nws)):
        assert bool((b[:pad] == fill).all()) and bool((b[pad + size:] == fill).all())
    got = buf[pad:pad + n].view(dtype).view(B, H * W, C)
    _close(got, _reference(shape, dtype, True, True), dtype)


@pytest.mark.parametrize("shape", [PLAIN[2], PLAIN[5], PLAIN[7], CAT[0]], ids=lambda s: "%dx%dg%d_%dx%d_ca%d" % s)
def test_gn_stream_cstats_is_deterministic(shape):
    """The one-kernel path folds its statistics in a fixed shape: two calls return the same bits, a replayed graph too."""
    path = "cstats_cat" if shape[5] else "cstats"
    dtype = torch.float16
    first = _run(path, shape, dtype, True, True)
    second = _run(path, shape, dtype, True, True)
    assert torch.equal(first, second)
    y = torch.zeros_like(first)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(path, shape, dtype, True, True, y.data_ptr())
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, y)
