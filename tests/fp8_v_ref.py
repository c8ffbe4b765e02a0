"""Reference quantiser / dequantiser of the FP8 (e4m3) V offload table, written from the contract in
f64 torch ops; it imports nothing of shadowkv_amd.

Token row v[0..D) (bf16, finite):
    amax  = max |v[d]|
    scale = the smallest power of two with amax / scale <= 448, clamped to [2^-100, 2^100]; amax == 0: scale = 1
    byte  = e4m3fn(RNE(clamp(v[d] / scale, -448, 448)))
    v'[d] = bf16(scale * e4m3(byte[d]))
"""
import torch

E4M3_MAX = 448.0
SCALE_MIN_EXP, SCALE_MAX_EXP = -100, 100


def row_scales(v):
    """v [..., D] -> f64 [...] power-of-two scale per row."""
    amax = v.double().abs().amax(dim=-1)
    m, e = torch.frexp(amax / E4M3_MAX)                      # quotient = m * 2^e, m in [0.5, 1): 2^e >= quotient, 2^(e-1) < it
    k = torch.where(m == 0.5, e - 1, e)                      # ... unless the quotient IS 2^(e-1)
    k = k.clamp(SCALE_MIN_EXP, SCALE_MAX_EXP)
    k = torch.where(amax > 0, k, torch.zeros_like(k))
    return torch.ldexp(torch.ones_like(amax), k)


def quantize_rows(v):
    """v [..., D] bf16 -> (bytes uint8 [..., D], scale f32 [...])."""
    scale = row_scales(v)
    x = (v.double() / scale.unsqueeze(-1)).clamp(-E4M3_MAX, E4M3_MAX)     # a division by a power of two: exact in f64
    # x is a bf16 number times a power of two: exact in f32 unless it is below the f32 normals, where it is far below half the
    # smallest e4m3 subnormal (2^-10) and becomes (signed) zero either way.  torch's f32 -> e4m3fn cast rounds to nearest even.
    b = x.float().to(torch.float8_e4m3fn)
    return b.view(torch.uint8), scale.float()


def e4m3_values(b):
    """uint8 [...] -> f64 values of the e4m3fn bytes."""
    return b.view(torch.float8_e4m3fn).double()


def dequantize_rows(b, scale):
    """(bytes uint8 [..., D], scale [...]) -> (v' bf16 [..., D], the f64 product before the cast)."""
    prod = e4m3_values(b) * scale.double().unsqueeze(-1)
    return prod.to(torch.bfloat16), prod


def e4m3_ulp(x):
    """Spacing of the e4m3fn numbers around |x| <= 448 (f64): 2^(e - 3) in the binade [2^e, 2^(e+1)), 2^-9 below 2^-6."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -6))         # |x| = m * 2^e with m in [0.5, 1): binade exponent e - 1
    return torch.ldexp(torch.ones_like(x), e - 1 - 3)


def pattern_rows(seed=0, D=128):
    """Every finite bf16 pattern (65,280 of them) shuffled into 510 rows of 128, plus the special rows: zeros, magnitudes
    around 1e-30, values up to 3e38.  Returns bf16 [510 + 1 + 4 + 4, 128]."""
    bits = torch.arange(65536, dtype=torch.int32)
    finite = bits[(bits & 0x7F80) != 0x7F80]
    assert finite.numel() == 65280
    g = torch.Generator().manual_seed(seed)
    perm = finite[torch.randperm(finite.numel(), generator=g)]
    rows = perm.to(torch.int16).view(torch.bfloat16).view(510, D)
    zero = torch.zeros(1, D, dtype=torch.bfloat16)
    tiny = (torch.randn(4, D, generator=g) * 1e-30).to(torch.bfloat16)
    huge = (torch.rand(4, D, generator=g) * 2 - 1).double().mul(3e38).to(torch.bfloat16)
    huge[0, 0] = 3e38
    huge[1] = huge[1] * 1e-8                                 # a row whose scale stays below the clamp
    return torch.cat((rows, zero, tiny, huge))


def sweep_rows(seed=1, D=128):
    """Gaussian rows scaled by 2^k, k = -130 .. 126 in steps of 2 (every scale exponent inside the clamp and both clamps), and
    rows whose largest magnitude sits exactly on, one bf16 step below and one above 448 * 2^k.  bf16 [129 + 3 * 9, 128]."""
    g = torch.Generator().manual_seed(seed)
    ks = torch.arange(-130, 127, 2)
    rows = torch.ldexp(torch.randn(ks.numel(), D, generator=g).double(), ks.unsqueeze(-1)).to(torch.bfloat16)
    edge = []
    for k in (-104, -100, -30, -1, 0, 1, 30, 100, 104):
        base = (torch.randn(3, D, generator=g).double() * 50).clamp(-400, 400) * 2.0 ** k
        base[0, 5], base[1, 5], base[2, 5] = 448 * 2.0 ** k, -446 * 2.0 ** k, 452 * 2.0 ** k     # bf16 numbers around 448
        edge.append(base.to(torch.bfloat16))
    return torch.cat([rows] + edge)
