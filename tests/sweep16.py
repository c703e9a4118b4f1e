"""Exhaustive 16-bit sweeps of the elementwise kernels: the input domains, fp64 references and error bounds that
tests/test_domain_sweep_cpu.py (emulations and mutants) and tests/test_domain_sweep_gpu.py (the kernels) share.

A 16-bit type has 65 536 bit patterns, so an elementwise kernel is judged at EVERY finite input instead of at random ones. The
bounds are stated in the quantities a kernel cannot avoid: one rounding to 16 bit (u / 2), a handful of fp32 roundings and the
1-ulp hardware reciprocal / exp2 (2^-20 relative), the polynomial erf's 1.5e-7 absolute error, the argument rounding of exp, and
fp32 denormals (not pinned). All arithmetic here is fp64 on the tensors' own device."""
import math

import numpy as np
import torch

V = (1.0, -0.75, 1.25 * 2.0 ** -7, -2.0 ** -14)     # value operands of the sweeps: |v| <= 1, so no product leaves the finite range
MANT = {torch.float16: 10, torch.bfloat16: 7}       # stored mantissa bits
EMIN = {torch.float16: -14, torch.bfloat16: -126}   # exponent of the smallest normal
_domains = {}


def domain(dtype):
    """Every finite bit pattern of `dtype` (fp16: 63 488, bf16: 65 280; +-0 and the subnormals included) in bit order, CPU tensor.
    Made once; callers must not write into it."""
    if dtype not in _domains:
        allbits = torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16).copy()).view(dtype)
        _domains[dtype] = allbits[torch.isfinite(allbits)].clone()
    return _domains[dtype]


def ulp16(x, dtype):
    """Spacing of `dtype` at |x| (x: fp64 tensor), as fp64: 2^(floor(log2 |x|) - mantissa bits), and below the smallest normal
    (0 included) the subnormal spacing, 2^-24 for fp16 and 2^-133 for bf16."""
    x = x.double().abs()
    _, ex = torch.frexp(x)                                   # |x| = m 2^ex, m in [0.5, 1): floor(log2 |x|) = ex - 1
    e = torch.where(x > 0, ex - 1, torch.full_like(ex, EMIN[dtype])).clamp(min=EMIN[dtype])
    return torch.exp2((e - MANT[dtype]).double())            # a power of two: exact


def normal_cdf64(g):
    """Phi(g) = (1 + erf(g / sqrt 2)) / 2, evaluated as erfc(-g / sqrt 2) / 2: the same function without the cancellation at g << 0."""
    return 0.5 * torch.special.erfc(-g.double() / math.sqrt(2.0))


def gelu64(g):
    """g * (1 + erf(g / sqrt 2)) / 2, the exact-erf GELU of the reference (F.gelu), in fp64."""
    return g.double() * normal_cdf64(g)


def gelu_grad64(g):
    """d gelu / d g = Phi(g) + g phi(g), phi the normal density."""
    g = g.double()
    return normal_cdf64(g) + g * torch.exp(-0.5 * g * g) / math.sqrt(2.0 * math.pi)


def silu64(z):
    """z / (1 + e^-z); e^-z overflows to +inf below z = -709 and the quotient is then -0: right to 2^-1000, and torch raises no warning."""
    z = z.double()
    return z / (1.0 + torch.exp(-z))


def _half_u(got, ref, dtype, rounding):
    """u / 2, u the 16-bit spacing at max(|got|, |ref|); rounding=False leaves the term out (a bound's allowance for everything but the
    final rounding, which the CPU emulations are judged against)."""
    return 0.5 * ulp16(torch.maximum(got.double().abs(), ref.double().abs()), dtype) if rounding else 0.0


def geglu_fwd_bound(got, ref, v, g, dtype, rounding=True):
    """out = v * gelu(g):  |got - ref| <= u / 2 + 2^-20 |ref| + 2^-21 |v| min(|g|, 8) + 2^-126.
    u / 2: the one rounding to 16 bit. 2^-20 |ref|: the fp32 roundings and the 1-ulp reciprocal / exp2. 2^-21 |g|: the polynomial
    erf's 1.5e-7 absolute error, halved for Phi, with a margin of four; beyond |g| = 8, 1 - erf is below 1e-15. 2^-126: fp32 denormals."""
    v, g = v.double().abs(), g.double().abs()
    return _half_u(got, ref, dtype, rounding) + 2.0 ** -20 * ref.double().abs() + 2.0 ** -21 * v * g.clamp(max=8.0) + 2.0 ** -126


def geglu_dgate_bound(got, ref, dy, a, g, dtype, rounding=True):
    """dg = dy * a * gelu'(g):  |got - ref| <= u / 2 + |dy a| (2^-20 |gelu'(g)| + 2^-21) + 2^-126 (2^-21: the erf error in Phi,
    absolute; g phi(g) is below 0.25 and carries only relative error). da = dy * gelu(g) takes geglu_fwd_bound with v := dy."""
    da = (dy.double() * a.double()).abs()
    return _half_u(got, ref, dtype, rounding) + da * (2.0 ** -20 * gelu_grad64(g).abs() + 2.0 ** -21) + 2.0 ** -126


def silu_bound(got, ref, z, dtype, rounding=True):
    """out = silu(z):  |got - ref| <= u / 2 + 2^-20 |ref| max(1, |z| / 4) + |z| 2^-125 + 2^-126.
    |z| / 4: the fast exp rounds its argument z log2 e to fp32, a relative error of the result that grows like |z| 2^-24.
    |z| 2^-125 and 2^-126: sigmoid values below 2^-126 and 16-bit subnormal inputs / outputs meet fp32 denormals, which are not pinned."""
    z = z.double().abs()
    return _half_u(got, ref, dtype, rounding) + 2.0 ** -20 * ref.double().abs() * (z / 4.0).clamp(min=1.0) + z * 2.0 ** -125 + 2.0 ** -126


def worst(got, ref, bound, where=None):
    """(max of |got - ref| / bound, its flat index, a line naming the place). `where`: dict name -> tensor of the same shape, printed at
    the worst element. A NaN anywhere (a NaN result, or inf - inf) counts as an infinite ratio, so no caller's `r <= 1` can lose it."""
    ratio = ((got.double() - ref.double()).abs() / bound).reshape(-1)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(torch.argmax(ratio))
    r = float(ratio[i])
    line = "worst err/bound %.4f at #%d: got %r ref %r" % (r, i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]))
    for k, t in (where or {}).items():
        line += " %s %r" % (k, float(t.reshape(-1)[i]))
    return r, i, line


def geglu_operands(dtype, gates_fixed=(1.0, -1.0, 0.5, -3.0)):
    """The points of a GEGLU sweep, (values, gates) as flat 16-bit CPU tensors: the whole domain as gate once per v in V, then the
    whole domain as value once per fixed gate (|gelu| < 1 there, so the product stays finite)."""
    d = domain(dtype)
    n = d.numel()
    vals = torch.cat([torch.full((n,), v, dtype=dtype) for v in V] + [d] * len(gates_fixed))
    gates = torch.cat([d] * len(V) + [torch.full((n,), g, dtype=dtype) for g in gates_fixed])
    return vals, gates


def tile_to(x, n):
    """x (1-D) repeated cyclically to n elements: how a sweep pads its last row."""
    return x.repeat((n + x.numel() - 1) // x.numel())[:n]
