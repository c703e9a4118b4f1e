"""A kernel's result must not depend on what ran before it, beyond what the project states.

Two forward kernels keep device-side words from call to call: the level-0 self-attention (sta.ops._SA_FLAGS: word 0 = calls the optimistic
loop still sits out) and the head-pair cross-attention kernel (sta.ops.proj_stats: word [0] the same for its optimistic softmax). The
optimistic and the standard path round differently, so the words decide a result's BITS. Pinned here: the words expire as documented and the
fresh bits come back; sta.ops.reset_adaptive_state() restores them in place (same tensor, same address: a captured graph keeps replaying
into live memory); self-attention calls on different streams do not steer each other.

Conventions of tests/test_kernel_gpu.py: fp64 softmax on the same 16-bit inputs, eps = 2^-8 (bf16) / 2^-11 (fp16), and only the bounds the
project already states — 4 eps (1 + |ref|) against fp64, 2 eps (1 + |std|) between the optimistic and the standard loop, the block golden's
8 eps max / 4 eps mean. Everything else is torch.equal or an integer. "fresh" = the result of a call right after a reset. The state is
driven by writing the state word (what a hostile call leaves, deterministically); one test makes a really hostile call.
Every test resets what it touches at its start and in a finally."""
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import golden_inputs as gi  # noqa: E402
from oracle import xattn_oracle as orc  # noqa: E402
from tests.test_kernel_gpu import _case  # noqa: E402

C, HEADS, D = 320, 8, 40
DTYPES = [torch.bfloat16, torch.float16]
LOG2E = 1.4426950408889634
# keys that follow one query each (tests/test_kernel_gpu.py's "spiked" recipe): the query's row maximum jumps at a late key, exp2 overflows
# in the optimistic pass and the query's workgroups (every head, every batch row) are flagged. Two query tiles of 8 at N = 1024 = a quarter
# of the workgroups, six of 16 at N = 2048 — more than the eighth that makes the next 64 calls sit out
SPIKES = {1024: ((700, 5), (990, 300)), 2048: ((700, 5), (990, 300), (1500, 600), (1900, 1000), (100, 1300), (400, 1700))}


def _eps(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11


@functools.lru_cache(maxsize=None)
def _sa_case(B, N, dtype, spiked=False):
    """(q, k, v^T) on the GPU and the fp64 softmax of the same 16-bit values; shared between tests, never written to."""
    bf = dtype == torch.bfloat16
    g = torch.Generator().manual_seed(7)
    q = torch.randn(B, N, C, generator=g)
    ramp = torch.arange(N).view(1, N, 1) / N
    k = torch.randn(B, N, C, generator=g) * ((0.3 + 2.7 * ramp) if bf else (0.8 + 0.5 * ramp))
    v = torch.randn(B, N, C, generator=g).to(dtype)
    if spiked:
        for key, px in SPIKES[N]:
            k[:, key] = (20.0 if bf else 3.0) * q[:, px]
    qs, k = (q * (D ** -0.5 * LOG2E)).to(dtype).cuda(), k.to(dtype).cuda()      # q in log2 units: scale = ln 2
    v = v.cuda()
    q64, k64, v64 = (t.double().view(B, N, HEADS, D).transpose(1, 2) for t in (qs, k, v))
    ref = (torch.softmax(q64 @ k64.transpose(-1, -2) * math.log(2.0), -1) @ v64).transpose(1, 2).reshape(B, N, C)
    torch.cuda.synchronize()
    return qs, k, v.transpose(1, 2).contiguous(), ref


def _sa(case, sfrag=False):
    from sta import ops
    q, k, vt, _ = case
    return ops.self_attention(q, k, vt, HEADS, ops.LN2, sfrag=sfrag)


def _sa_standard(case, sfrag=False):
    from sta import ops
    ops.SELFATTN_OPTIMISTIC = False
    try:
        return _sa(case, sfrag)
    finally:
        ops.SELFATTN_OPTIMISTIC = True


def _sa_key(B, N, stream=None):
    from sta import lib
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    return (dev, stream.cuda_stream, lib.load().sta_selfattn_optimistic_flags_bytes(B, N, HEADS))


def _sa_words(key):
    from sta import ops
    return ops._SA_FLAGS[key].view(torch.int32)


def _word0(words):
    torch.cuda.synchronize()
    return int(words[0])


def _ratio(err, bound):
    return (err / bound).max().item()


def _inside_both(what, out, fresh, ref, dtype, sfrag=False):
    """`out` came from the standard loop (a call that sat out), `fresh` from the optimistic one: 2 eps (1 + |std|) apart, and `out` within
    4 eps (1 + |ref|) of the fp64 softmax."""
    from sta import ops
    eps = _eps(dtype)
    assert torch.isfinite(out).all()
    r_std = _ratio((out.float() - fresh.float()).abs(), 2 * eps * (1.0 + out.float().abs()))
    o = ops.from_sfrag(out) if sfrag else out
    r_ref = _ratio((o.double() - ref).abs(), 4 * eps * (1.0 + ref.abs()))
    print("%s: %.3f of the 2 eps bound against the fresh bits, %.3f of the 4 eps bound against fp64" % (what, r_std, r_ref))
    assert r_std <= 1.0 and r_ref <= 1.0, (what, r_std, r_ref)


def _supported(N):
    from sta import lib, ops
    assert ops.SELFATTN_OPTIMISTIC
    for code in (lib.STA_BF16, lib.STA_F16):
        assert lib.load().sta_selfattn_optimistic_supported(N, C, HEADS, ops.LN2, code)


# ------------------------------------------------------------------------------------------------------------ level-0 self-attention

@pytest.mark.parametrize("sfrag", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_selfattn_sit_out_expires_and_the_fresh_bits_return(dtype, sfrag):
    """State word n > 0: exactly n calls take the standard loop (inside both bounds, the bits of the standard kernel), the word counts
    down to 0, and call n + 1 gives the fresh bits again; 64 -> 63 in one call."""
    from sta import ops
    B, N = 2, 1024
    _supported(N)
    case = _sa_case(B, N, dtype)
    ref = case[3]
    ops.reset_adaptive_state()
    try:
        a0 = _sa(case, sfrag)
        words = _sa_words(_sa_key(B, N))
        assert _word0(words) == 0 and int(words[1]) == 0
        std = _sa_standard(case, sfrag)
        _inside_both("fresh", a0, a0, ref, dtype, sfrag)                # (the fresh bits themselves against fp64)
        words[0] = 1
        o = _sa(case, sfrag)
        assert _word0(words) == 0
        assert torch.equal(o, std), "a call that sits out runs the standard loop"
        _inside_both("sat out (1)", o, a0, ref, dtype, sfrag)
        assert torch.equal(_sa(case, sfrag), a0), "the call after the sit-out expired does not give the fresh bits"
        words[0] = 2
        o1, o2, o3 = _sa(case, sfrag), _sa(case, sfrag), _sa(case, sfrag)
        assert _word0(words) == 0
        for i, o in enumerate((o1, o2)):
            assert torch.equal(o, std)
            _inside_both("sat out (2, call %d)" % (i + 1), o, a0, ref, dtype, sfrag)
        assert torch.equal(o3, a0)
        words[0] = 64
        _sa(case, sfrag)
        assert _word0(words) == 63
    finally:
        ops.reset_adaptive_state()


@pytest.mark.parametrize("dtype", DTYPES)
def test_selfattn_hostile_call_then_reset_restores_the_fresh_bits_in_place(dtype):
    """From real inputs to the state: a call whose keys make a quarter of the workgroups overflow leaves word 0 = 64; the same friendly
    call behind it is inside both bounds (not necessarily the fresh bits); reset_adaptive_state() zeroes the SAME buffer and the fresh
    bits are back."""
    from sta import ops
    B, N = 2, 1024
    _supported(N)
    case, hostile = _sa_case(B, N, dtype), _sa_case(B, N, dtype, True)
    key = _sa_key(B, N)
    ops.reset_adaptive_state()
    try:
        a0 = _sa(case)
        h = _sa(hostile)
        words = _sa_words(key)
        assert _word0(words) == 64 and int(words[1]) == 0, words[:2].tolist()
        eps = _eps(dtype)
        assert _ratio((h.double() - hostile[3]).abs(), 4 * eps * (1.0 + hostile[3].abs())) <= 1.0      # the hostile call itself is exact
        o = _sa(case)
        assert _word0(words) == 63
        _inside_both("behind the hostile call", o, a0, case[3], dtype)
        buf = ops._SA_FLAGS[key]
        ptr = buf.data_ptr()
        assert int(buf.count_nonzero()) > 0
        ops.reset_adaptive_state()
        assert ops._SA_FLAGS[key] is buf and buf.data_ptr() == ptr, "the reset must keep the buffer (captured graphs hold its address)"
        assert int(buf.count_nonzero()) == 0
        assert torch.equal(_sa(case), a0)
        assert _word0(words) == 0
    finally:
        ops.reset_adaptive_state()


@pytest.mark.parametrize("dtype", DTYPES)
def test_selfattn_shapes_that_share_a_flags_buffer(dtype):
    """(B, N) = (2, 1024) and (1, 2048) have the same flags size, hence ONE cache entry: a hostile call at one shape must not reach the
    other one through it — inside the fp64 bound while the entry sits out (the per-workgroup words are those of another grid), the
    fresh bits after a reset."""
    from sta import ops
    shapes = [(2, 1024), (1, 2048)]
    assert _sa_key(*shapes[0]) == _sa_key(*shapes[1])
    eps = _eps(dtype)
    ops.reset_adaptive_state()
    try:
        for host, friend in (shapes, shapes[::-1]):
            _supported(friend[1])
            case, hostile = _sa_case(*friend, dtype), _sa_case(*host, dtype, True)
            fresh = _sa(case)
            words = _sa_words(_sa_key(*friend))
            assert _word0(words) == 0
            assert _ratio((fresh.double() - case[3]).abs(), 4 * eps * (1.0 + case[3].abs())) <= 1.0
            _sa(hostile)
            assert _word0(words) == 64, (host, words[:2].tolist())
            o = _sa(case)                                  # sits out on the other shape's leftovers
            assert _word0(words) == 63
            _inside_both("%s behind a hostile %s" % (friend, host), o, fresh, case[3], dtype)
            ops.reset_adaptive_state()
            o = _sa(case)
            assert torch.equal(o, fresh), (host, friend)
            assert _word0(words) == 0
    finally:
        ops.reset_adaptive_state()


@pytest.mark.parametrize("dtype", DTYPES)
def test_selfattn_streams_do_not_steer_each_other(dtype):
    """One cache entry per stream: a stream that sits out leaves another stream's bits and words alone."""
    from sta import ops
    B, N = 2, 1024
    _supported(N)
    case = _sa_case(B, N, dtype)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    k1, k2 = _sa_key(B, N, s1), _sa_key(B, N, s2)
    assert k1 != k2 and _sa_key(B, N) not in (k1, k2)
    ops.reset_adaptive_state()
    try:
        a0 = _sa(case)
        torch.cuda.synchronize()

        def on(stream):
            with torch.cuda.stream(stream):
                return _sa(case)

        o1, o2 = on(s1), on(s2)
        s1.synchronize()
        s2.synchronize()
        assert k1 in ops._SA_FLAGS and k2 in ops._SA_FLAGS
        assert ops._SA_FLAGS[k1] is not ops._SA_FLAGS[k2] and ops._SA_FLAGS[k1].data_ptr() != ops._SA_FLAGS[k2].data_ptr()
        assert torch.equal(o1, a0) and torch.equal(o2, a0)
        with torch.cuda.stream(s1):
            _sa_words(k1)[0] = 64
        s1.synchronize()
        before = _sa_words(k2).clone()
        o1, o2 = on(s1), on(s2)
        s1.synchronize()
        s2.synchronize()
        assert torch.equal(o2, a0), "a sit-out on one stream changed another stream's bits"
        assert torch.equal(_sa_words(k2), before)
        assert int(_sa_words(k1)[0]) == 63
        _inside_both("the stream that sits out", o1, a0, case[3], dtype)
    finally:
        ops.reset_adaptive_state()


def test_selfattn_captured_graph_replays_into_the_live_buffer():
    """A call captured on a stream that already has its flags buffer holds the buffer's address: replays read and advance the live words,
    a reset between replays takes effect in place, and a reset INSIDE a capture is refused with the words untouched."""
    from sta import ops
    B, N, dtype = 2, 1024, torch.float16
    _supported(N)
    case = _sa_case(B, N, dtype)
    s = torch.cuda.Stream()
    key = _sa_key(B, N, s)
    ops.reset_adaptive_state()
    try:
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            a0 = _sa(case)                       # warm-up on the capturing stream: makes (or finds) the buffer, fresh bits
        s.synchronize()
        buf = ops._SA_FLAGS[key]
        ptr, words = buf.data_ptr(), _sa_words(key)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = _sa(case)
        assert ops._SA_FLAGS[key] is buf

        def replay():
            g.replay()
            torch.cuda.synchronize()
            return out.clone()

        assert torch.equal(replay(), a0)
        words[0] = 2
        r1, r2, r3 = replay(), replay(), replay()
        _inside_both("replay 1 of a sit-out of 2", r1, a0, case[3], dtype)
        _inside_both("replay 2 of a sit-out of 2", r2, a0, case[3], dtype)
        assert torch.equal(r3, a0) and _word0(words) == 0
        words[0] = 64
        replay()                                            # sits out, 63 left: the reset below must undo it
        assert _word0(words) == 63
        ops.reset_selfattn_optimistic_state()
        assert ops._SA_FLAGS[key] is buf and buf.data_ptr() == ptr
        assert torch.equal(replay(), a0), "a reset between replays did not reach the captured call"
        assert _word0(words) == 0
        words[0] = 5
        torch.cuda.synchronize()
        before = words.clone()
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=s):
            for reset in (ops.reset_selfattn_optimistic_state, ops.reset_proj_stats, ops.reset_adaptive_state):
                with pytest.raises(RuntimeError, match="captur"):
                    reset()
            _sa(case)
        torch.cuda.synchronize()
        assert torch.equal(words, before) and ops._SA_FLAGS[key] is buf and buf.data_ptr() == ptr
    finally:
        ops.reset_adaptive_state()


# ------------------------------------------------------------------------------------------------ head-pair cross-attention (level 0)

P_N, P_K, P_I = 1024, 2, 2


@functools.lru_cache(maxsize=None)
def _proj_case(dtype):
    """Friendly logits (the inputs of test_fwd_proj_pair_extreme_logits without the extreme part), y in query-fragment order, and the
    oracle fed q = round16(y Wq^T) per image; shared, never written to."""
    from sta import ops
    dev = "cuda"
    g = torch.Generator().manual_seed(5)
    wq = (torch.randn(C, C, generator=g) / math.sqrt(C)).to(dtype)
    cases = [_case(P_N, C, HEADS, P_K, dtype, seed=90 + i) for i in range(P_I)]
    y = torch.cat([c[0] for c in cases]).to(dev)
    k = torch.cat([c[1] for c in cases]).to(dev)
    v = torch.cat([c[2] for c in cases]).to(dev)
    mb = torch.stack([ops.mask_bits(c[3]) for c in cases]).to(dev)
    coef = torch.stack([c[4] for c in cases]).to(dev)
    scale = D ** -0.5
    refs = []
    for yi, ki, vi, mi, ci in cases:
        q16 = (yi.double() @ wq.double().t()).to(dtype)
        refs.append(orc.fused_xattn(q16.double(), ki.double(), vi.double(), mi, ci.double(), HEADS, scale))
    args = (ops.to_qfrag(y), ops.pack_wq(wq.to(dev), HEADS), ops.pack_kv_proj(k, v, HEADS, n_img=P_I), mb, coef, scale)
    torch.cuda.synchronize()
    return args, torch.cat(refs)


def _proj(case, stats):
    from sta import ops
    return ops.xattn_forward_proj(*case[0], qfrag=True, ofrag=True, stats=stats)


def _proj_inside_both(what, out, fresh, ref, dtype):
    from sta import ops
    eps = _eps(dtype)
    assert torch.isfinite(out).all()
    r_std = _ratio((out.float() - fresh.float()).abs(), 2 * eps * (1.0 + fresh.float().abs()))
    r_ref = _ratio((ops.from_ofrag(out).float().cpu().double() - ref).abs(), 4 * eps * (1.0 + ref.abs()))
    print("%s: %.3f of the 2 eps bound against the fresh bits, %.3f of the 4 eps bound against the oracle" % (what, r_std, r_ref))
    assert r_std <= 1.0 and r_ref <= 1.0, (what, r_std, r_ref)


def _st(stats):
    torch.cuda.synchronize()
    return stats.cpu().tolist()


@pytest.mark.parametrize("dtype", DTYPES)
def test_proj_pair_sit_out_expires_and_the_fresh_bits_return(dtype):
    """The default statistics buffer of the stream: word [0] = n > 0 makes exactly n launches take the standard softmax (inside both
    bounds, word [7] counts them), launch n + 1 gives the fresh bits; reset_proj_stats() zeroes the 8 words in place."""
    from sta import lib, ops
    case = _proj_case(dtype)
    ref = case[1]
    lib.set_option(lib.OPT_PROJ_PAIR, 1)
    ops.reset_adaptive_state()
    try:
        fresh = _proj(case, None)
        _proj_inside_both("fresh", fresh, fresh, ref, dtype)
        stats = ops.proj_stats()
        assert stats is not None and stats.numel() == lib.P3_STATS_WORDS and _st(stats) == [0] * lib.P3_STATS_WORDS
        assert torch.equal(_proj(case, True), fresh)
        s = _st(stats)
        assert s[0] == 0 and s[1:4] == [0, 0, 0] and s[4] > 0 and s[6] == 1 and s[7] == 0, s
        stats[0] = 1
        o = _proj(case, True)
        s1 = _st(stats)
        assert s1[0] == 0 and s1[7] == 1 and s1[6] == 2 and s1[4] == s[4], s1      # sat out: nothing evaluated optimistically
        _proj_inside_both("sat out (1)", o, fresh, ref, dtype)
        assert torch.equal(_proj(case, True), fresh), "the launch after the sit-out expired does not give the fresh bits"
        stats[0] = 2
        o1, o2, o3 = _proj(case, True), _proj(case, True), _proj(case, True)
        s2 = _st(stats)
        assert s2[0] == 0 and s2[7] == 3 and s2[6] == 6, s2
        _proj_inside_both("sat out (2, launch 1)", o1, fresh, ref, dtype)
        _proj_inside_both("sat out (2, launch 2)", o2, fresh, ref, dtype)
        assert torch.equal(o1, o2) and torch.equal(o3, fresh)
        stats[0] = 64
        _proj(case, True)
        assert _st(stats)[0] == 63
        ptr = stats.data_ptr()
        ops.reset_proj_stats()
        assert ops.proj_stats() is stats and stats.data_ptr() == ptr
        assert _st(stats) == [0] * lib.P3_STATS_WORDS
        assert torch.equal(_proj(case, True), fresh)
    finally:
        lib.set_option(lib.OPT_PROJ_PAIR, 0)
        ops.reset_adaptive_state()


# ------------------------------------------------------------------------------------------ one level-0 block: both kernels in one chain

@pytest.mark.parametrize("dtype", DTYPES)
def test_block_chain_returns_to_its_fresh_bits_after_a_reset(dtype, monkeypatch):
    """The level-0 chain of tests/test_modules_gpu.py::test_block_projection_fused_path_vs_reference_golden (pair = True; block_d40.npz:
    N = 256, C = 320, K = 2) runs BOTH stateful kernels: fresh, with both state words at 64, after reset_adaptive_state(). Every output
    meets the golden's bound, the third is the first bit for bit."""
    from ldm.modules.attention import BasicTransformerBlock
    from sta import fused, lib, ops, prompt_state
    from sta.synth import seeded_fill_
    monkeypatch.setattr(ops, "PROJ_MIN_WORKGROUPS", 0)
    monkeypatch.setattr(fused, "ROWGEMM_MIN_ROWS", 0)
    lib.set_option(lib.OPT_PROJ_PAIR, 1)          # reset after the test by conftest
    g = np.load(os.path.join(gi.GOLDEN, "block_d40.npz"), allow_pickle=False)
    dim, C_, heads, K, seed = (int(g[k]) for k in ("dim", "C", "heads", "K", "seed"))
    assert (C_, heads) == (C, HEADS)
    x, context, local_ctx = gi.block_inputs(dim, C_, K, seed, gi.load_uncond())
    blk = BasicTransformerBlock(C_, heads, C_ // heads, context_dim=768, checkpoint=False)
    seeded_fill_(blk, seed)
    blk = blk.to("cuda", dtype)
    x, context = x.cuda().to(dtype), context.cuda().to(dtype)
    coef, boxes = torch.from_numpy(g["coef"]).cuda(), [list(c) for c in g["centres"]]
    prompt_state.begin_prompt([c.cuda() for c in local_ctx], first_timestep=981)
    ref = g["out"]
    eps = _eps(dtype)

    def run(what):
        with torch.no_grad():
            out = blk(x, context=context, time=torch.tensor(981), coef=coef, bboxs_curr=boxes)
        torch.cuda.synchronize()
        err = np.abs(out.float().cpu().numpy() - ref)
        print("%s: max %.3f of 8 eps max|ref|, mean %.3f of 4 eps mean|ref|"
              % (what, err.max() / (8 * eps * np.abs(ref).max()), err.mean() / (4 * eps * np.abs(ref).mean())))
        assert err.max() <= 8 * eps * np.abs(ref).max(), (what, err.max(), np.abs(ref).max())
        assert err.mean() <= 4 * eps * np.abs(ref).mean(), (what, err.mean(), np.abs(ref).mean())
        return out

    key = _sa_key(x.shape[0], dim * dim, None)
    ops.reset_adaptive_state()
    try:
        launches = int(ops.proj_stats()[6])
        first = run("fresh")
        assert key in ops._SA_FLAGS, "the block did not take the optimistic self-attention kernel"
        stats, words = ops.proj_stats(), _sa_words(key)
        assert int(stats[6]) == launches + 1, "the block did not take the head-pair kernel with the stream's statistics words"
        assert _word0(words) == 0 and int(stats[0]) == 0
        words[0] = 64
        stats[0] = 64
        run("both kernels sitting out")
        assert _word0(words) == 63 and int(stats[0]) == 63
        ops.reset_adaptive_state()
        third = run("after the reset")
        assert torch.equal(third, first)
        assert _word0(words) == 0 and int(stats[0]) == 0
    finally:
        ops.reset_adaptive_state()
