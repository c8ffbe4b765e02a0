"""Tensor-op surface the reference's host models import (`/root/reference/models/tensor_op.py`),
re-implemented on PyTorch-ROCm ops + libshadowkv_hip.so.

Names, argument order and return values follow the reference so `models/llama.py` /
`models/base.py`-style host code can import from here unchanged:
  layer_norm, apply_rotary_pos_emb, apply_rotary_pos_emb_single, apply_rotary_pos_emb_cuda,
  apply_rotary_pos_emb_cuda_push_cache, batch_gather_gemm_rotary_pos_emb_cuda, sample_token, ...
plus what replaces third-party CUDA packages on this path:
  sparse_attention_decode  (flash_attn_with_kvcache at base.py:341, q_len == 1)
  causal_attention_prefill (flash_attn_with_kvcache(causal=True) at base.py:293 / :311, the prompt)
  minference_prefill_kernel (MInference vertical + slash sparse prefill, tensor_op.py:68-117)
  silu_and_mul, rotary_embedding_neox  (vllm._custom_ops at llama.py:296,421)
"""
import math

import torch
import torch.nn.functional as F

from ._lib import lib, check, ptr, current_stream_handle, KvProjDesc, KV_PROJ_IN_SCAN, KV_PROJ_IN_TOPK  # noqa: F401
from .kernels import shadowkv


# ---------------------------------------------------------------------------- norms / activations
def layer_norm(hidden_states, eps, w):
    """RMSNorm (reference: flashinfer.norm.rmsnorm, tensor_op.py:34-39; the commented-out torch
    version at :41-51 is the spec: f32 variance, normalise, cast back, scale by w)."""
    shape = hidden_states.shape
    out = F.rms_norm(hidden_states.reshape(-1, shape[-1]), (shape[-1],), w, eps)
    return out.view(shape)


def silu_and_mul(out, x):
    """out = silu(x[..., :d]) * x[..., d:]  (vllm._custom_ops.silu_and_mul, llama.py:421)."""
    d = x.shape[-1] // 2
    torch.mul(F.silu(x[..., :d]), x[..., d:], out=out)
    return out


# ---------------------------------------------------------------------------- weight-only FP8
FP8_MAX = 448.0       # largest finite e4m3fn value


def quantize_fp8_rows(w, pow2_scale=False):
    """(w8, scale): w [N, K] -> e4m3fn bytes [N, K] (torch.float8_e4m3fn, the OCP encoding) and one f32 scale per row with
    w[n][k] ~ scale[n] * e4m3(w8[n][k]).  scale[n] = max|w[n]| / 448 (pow2_scale: rounded UP to a power of two, so that
    scale * e4m3 is a bf16 number); an all-zero row gets scale 1.  The quotient is clamped to +-448 before the cast - torch's
    cast does not saturate (500 -> the NaN byte 0x7F) - so no 0x7F / 0xFF byte is ever produced.  Host-side torch ops only."""
    if w.dim() != 2:
        raise ValueError("quantize_fp8_rows takes a [N, K] matrix")
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    scale = amax / FP8_MAX
    if pow2_scale:
        m, e = torch.frexp(scale.clamp_min(2.0 ** -126))        # scale = m * 2^e, m in [0.5, 1): exact, unlike log2
        scale = torch.ldexp(torch.ones_like(scale), torch.where(m == 0.5, e - 1, e))
    # (a row whose largest magnitude is below the smallest normal f32 * 448 is quantised against scale 2^-126: still finite)
    scale = torch.where(amax > 0, scale.clamp_min(2.0 ** -126), torch.ones_like(scale))
    w8 = (wf / scale.unsqueeze(1)).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return w8.contiguous(), scale.contiguous()


def dequantize_fp8_rows(w8, scale, dtype=torch.bfloat16):
    """scale[n] * e4m3(w8[n][k]) as `dtype` (one f32 multiply, one rounding): what prefill, the FP8 fallbacks and the tests use."""
    return (w8.float() * scale.float().unsqueeze(1)).to(dtype)


# ---------------------------------------------------------------------------- FP8 V offload table
V_DTYPES = ("bf16", "fp8_e4m3")
LANDMARK_DTYPES = ("bf16", "fp8_e4m3")             # the landmark table of the decode scan: same rule, per landmark row
V_SCALE_MIN_EXP, V_SCALE_MAX_EXP = -100, 100


def quantize_v_rows_torch(v):
    """Torch mirror of skv_quantize_v_rows (any device): v [..., D] -> (e4m3fn bytes [..., D], f32 scale [...]) per token row:
    scale = the smallest power of two with max|v| / scale <= 448, clamped to [2^-100, 2^100], 1 for an all-zero row;
    byte = e4m3fn(RNE(clamp(v / scale, -448, 448))).  Rows with NaN / Inf are outside the contract."""
    vf = v.float()
    amax = vf.abs().amax(dim=-1)
    m, e = torch.frexp(amax)                               # amax = m * 2^e, m in [0.5, 1); 448 = 0.875 * 2^9
    k = torch.where(m <= 0.875, e - 9, e - 8).clamp(V_SCALE_MIN_EXP, V_SCALE_MAX_EXP)
    k = torch.where(amax > 0, k, torch.zeros_like(k))
    one = torch.ones_like(amax)
    scale, inv = torch.ldexp(one, k), torch.ldexp(one, -k)
    v8 = (vf * inv.unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return v8, scale


def dequantize_v_rows(v8, scale, dtype=torch.bfloat16):
    """scale * e4m3(byte) per token row: v8 [..., D] float8_e4m3fn, scale [...] f32.  The product is a bf16 number (exact)."""
    return (v8.float() * scale.unsqueeze(-1)).to(dtype)


def quantize_v_rows(v, table, scale):
    """skv_quantize_v_rows: v bf16 [bs, kv, T, 128] (any strides with a contiguous last dimension - the transposed view of a
    fused QKV output is taken as it is, nothing is copied) -> table [bs, kv, >= T * 128] bytes / float8 and scale
    [bs, kv, >= T] f32, both views whose (batch, head) blocks are evenly spaced and whose rows are contiguous."""
    bs, kv, T, D = v.shape
    tb, sb = table.reshape(bs, kv, -1) if table.dim() != 3 else table, scale.reshape(bs, kv, -1) if scale.dim() != 3 else scale
    if tb.data_ptr() != table.data_ptr() or sb.data_ptr() != scale.data_ptr():
        raise ValueError("table / scale must be views with contiguous rows per (batch, head)")
    if v.dtype != torch.bfloat16 or v.stride(3) != 1 or tb.element_size() != 1 or sb.dtype != torch.float32:
        raise ValueError("quantize_v_rows takes bf16 rows, a byte table and f32 scales")
    if tb.stride(2) != 1 or sb.stride(2) != 1 or (bs > 1 and (tb.stride(0) != kv * tb.stride(1) or sb.stride(0) != kv * sb.stride(1))):
        raise ValueError("table / scale blocks must be evenly spaced over (batch, head)")
    if tb.shape[2] < T * D or sb.shape[2] < T:
        raise ValueError("table / scale rows are shorter than the token rows to quantise")
    check(lib().skv_quantize_v_rows(ptr(v), v.stride(0), v.stride(1), v.stride(2), bs, kv, T, D, ptr(tb), tb.stride(1),
                                    ptr(sb), sb.stride(1), current_stream_handle()), "quantize_v_rows")


# ---------------------------------------------------------------------------- weight-only MXFP4
MXFP4_BLOCK = 32                                   # elements that share one e8m0 scale byte (OCP MX)
MXFP4_MIN_K = 1024                                 # smallest K of the native GEMV
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)     # e2m1 codes 0..7; bit 3 of a nibble is the sign


def quantize_mxfp4_rows(w):
    """(w4, w_scale): w [N, K], K % 32 == 0 -> uint8 [N, K / 2] (element 2i in the low nibble of byte i, element 2i + 1 in the
    high nibble; nibble = sign bit + e2m1 code) and uint8 e8m0 scales [N, K / 32], one per 32 consecutive elements of a row:
    w[n][k] ~ 2^(w_scale[n][k / 32] - 127) * e2m1(nibble[n][k]).  Per block the scale is the smallest power of two 2^s with
    max|w| / 2^s <= 6 (frexp, as quantize_v_rows_torch: nothing is ever clipped), s clamped to [-100, 100] (bytes 27..227; an
    all-zero block: s = 0); elements are w / 2^s rounded to the nearest e2m1 value, ties to the even mantissa.  Rows with
    NaN / Inf are outside the contract.  Torch ops only, any device."""
    if w.dim() != 2 or w.shape[1] % MXFP4_BLOCK:
        raise ValueError(f"quantize_mxfp4_rows takes a [N, K] matrix with K % {MXFP4_BLOCK} == 0")
    N, K = w.shape
    wf = w.float().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = wf.abs().amax(dim=-1)
    m, e = torch.frexp(amax)                               # amax = m * 2^e, m in [0.5, 1); 6 = 0.75 * 2^3
    s = torch.where(m <= 0.75, e - 3, e - 2).clamp(V_SCALE_MIN_EXP, V_SCALE_MAX_EXP)
    s = torch.where(amax > 0, s, torch.zeros_like(s))
    inv = ((127 - s).to(torch.int32) << 23).view(torch.float32)     # 2^-s from its bits: exact on every device
    a = wf.abs() * inv.unsqueeze(-1)                      # (a block whose max is below 2^-100's reach rounds towards 0)
    # nearest e2m1 value, ties to the even mantissa: the grid step is 0.5 below 2, 1 in [2, 4), 2 in [4, 6]; torch.round is RNE
    # and the even multiples of each step are the codes with mantissa bit 0
    q = torch.where(a < 2, torch.round(a * 2) * 0.5, torch.where(a < 4, torch.round(a), torch.round(a * 0.5) * 2)).clamp_max(6.0)
    code = torch.where(q < 2, q * 2, torch.where(q < 4, q + 2, q * 0.5 + 4)).to(torch.uint8)
    nib = (code | ((wf < 0).to(torch.uint8) << 3)).reshape(N, K // 2, 2)
    w4 = nib[..., 0] | (nib[..., 1] << 4)
    return w4.contiguous(), (s + 127).to(torch.uint8).contiguous()


def dequantize_mxfp4_rows(w4, w_scale, dtype=torch.bfloat16):
    """2^(w_scale - 127) * e2m1(nibble) as `dtype` [N, K]: what prefill, the MXFP4 fallbacks and the tests use.  Every value has
    2 significant bits: exact in bf16 for scale bytes 27..227."""
    _mxfp4_check(w4, w_scale)
    N = w4.shape[0]
    nib = torch.stack((w4 & 0xF, w4 >> 4), dim=-1).reshape(N, -1).long()
    mag = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=w4.device)[nib & 7]
    val = torch.where((nib & 8) != 0, -mag, mag).reshape(N, -1, MXFP4_BLOCK)
    scale = (w_scale.to(torch.int32) << 23).view(torch.float32)     # 2^(byte - 127) from its bits
    return (val * scale.unsqueeze(-1)).reshape(N, -1).to(dtype)


def _mxfp4_check(w, w_scale):
    if w.dtype != torch.uint8 or w.dim() != 2:
        raise ValueError("MXFP4 weights are a uint8 [N, K / 2] tensor of packed e2m1 nibbles")
    N, K = w.shape[0], 2 * w.shape[1]
    if K % MXFP4_BLOCK or w_scale is None or w_scale.dtype != torch.uint8 or tuple(w_scale.shape) != (N, K // MXFP4_BLOCK):
        raise ValueError(f"MXFP4 weights uint8 [N, K / 2] = {tuple(w.shape)} go with e8m0 scales uint8 [N, K / 32] = "
                         f"({N}, {K // MXFP4_BLOCK}) with K % 32 == 0, got "
                         f"{None if w_scale is None else (w_scale.dtype, tuple(w_scale.shape))}")


def _mxfp4_check_x(x, w, w_scale):
    _mxfp4_check(w, w_scale)
    if x.shape[-1] != 2 * w.shape[1]:
        raise ValueError(f"x [..., K] with K = {x.shape[-1]} does not match MXFP4 weights uint8 [N, K / 2] = {tuple(w.shape)} "
                         f"and scales uint8 [N, K / 32]")


def _fp8_check_x(x, w, w_scale):
    if w.dtype != torch.float8_e4m3fn:
        raise ValueError("w_scale goes with float8_e4m3fn weights")
    if w_scale.dtype != torch.float32 or w_scale.numel() != w.shape[0] or not w_scale.is_contiguous():
        raise ValueError("w_scale must be a contiguous f32 vector with one entry per weight row")


# ---------------------------------------------------------------------------- decode projections: one dispatch, three weight formats
MAX_GEMV_ROWS = 32   # token rows served by the native kernels (1: GEMV, 2..32: small-M MFMA kernel); more -> F.linear
FP8_ROWS_MODES = ("fallback", "native")      # what 2..MAX_GEMV_ROWS token rows against FP8 weights take (linear_decode)
MXFP4_ROWS_MODES = ("fallback", "native")    # what 2..MAX_GEMV_ROWS token rows against an MXFP4 pair take (linear_decode)

fp8_native_calls = 0      # native FP8 launches / dequantising fallbacks taken so far (diagnostics; the tests read them)
fp8_fallback_calls = 0
mxfp4_native_calls = 0    # the same for MXFP4
mxfp4_fallback_calls = 0


class _WeightFormat:
    """What differs between the weight formats of the decode projections; everything else is the one path of linear_decode,
    norm_linear_decode and norm_qkv_rope_update.  Three records, built once below; a call only reads one.
      weight_dtype              the name DecoderLM knows the format by
      gemv, gemv_near_pull, norm_gemv, norm_gemv_rangemax, norm_gemv_near_pull, linear_rows, qkv_gemv_rope_update
                                the symbol of the format's native entry of each kind ("skv_" + kind + suffix)
      validate(x, w, w_scale)   raises ValueError for a (w, w_scale) pair the format does not take; None: nothing to check
      scaled                    w_scale follows w in every native call; the scaled formats are the counted ones
      k_step, k_min             one token row is native with K % k_step == 0 and K >= k_min and contiguous x and w -
      scale_contiguous          - and, where set, a contiguous w_scale
      rows_k_step, rows_k_min   2..MAX_GEMV_ROWS token rows are native with K % rows_k_step == 0, K >= rows_k_min, the same
      rows_keyword, rows_gpu    contiguity, the keyword of this name (None: always) set to "native", and, where rows_gpu, x.is_cuda
      quantize(w, pow2_scale), dequantize(w, w_scale, dtype)    bf16 <-> the format (None: bf16 itself)
      native_counter, fallback_counter                          names of the module's call counters (None: bf16, not counted)"""
    KINDS = ("gemv", "gemv_near_pull", "norm_gemv", "norm_gemv_rangemax", "norm_gemv_near_pull", "linear_rows", "qkv_gemv_rope_update")
    __slots__ = KINDS + ("weight_dtype", "what", "validate", "scaled", "k_step", "k_min", "scale_contiguous", "rows_k_step", "rows_k_min",
                         "rows_keyword", "rows_gpu", "quantize", "dequantize", "native_counter", "fallback_counter")

    def __init__(self, weight_dtype, suffix, what_suffix, qkv_suffix, **fields):
        self.weight_dtype = weight_dtype
        self.what = {}                  # symbol -> the name a native error carries (bf16: the kind alone)
        for kind in self.KINDS:
            qkv = kind == "qkv_gemv_rope_update"
            setattr(self, kind, "skv_" + kind + (qkv_suffix if qkv else suffix))
            self.what[getattr(self, kind)] = kind + (qkv_suffix if qkv else what_suffix)
        for name, value in fields.items():
            setattr(self, name, value)


_BF16 = _WeightFormat("bf16", "_bf16", "", "", validate=None, scaled=False, k_step=32, k_min=512, scale_contiguous=False,
                      rows_k_step=32, rows_k_min=512, rows_keyword=None, rows_gpu=False, quantize=None, dequantize=None,
                      native_counter=None, fallback_counter=None)
_FP8 = _WeightFormat("fp8_e4m3", "_fp8", "_fp8", "_fp8", validate=_fp8_check_x, scaled=True, k_step=16, k_min=1024, scale_contiguous=False,
                     rows_k_step=64, rows_k_min=0, rows_keyword="fp8_rows", rows_gpu=False,
                     quantize=quantize_fp8_rows, dequantize=dequantize_fp8_rows,
                     native_counter="fp8_native_calls", fallback_counter="fp8_fallback_calls")
_MXFP4 = _WeightFormat("mxfp4", "_mxfp4", "_mxfp4", "_mxfp4", validate=_mxfp4_check_x, scaled=True, k_step=MXFP4_BLOCK, k_min=MXFP4_MIN_K,
                       scale_contiguous=True, rows_k_step=128, rows_k_min=0, rows_keyword="mxfp4_rows", rows_gpu=True,
                       quantize=lambda w, pow2_scale=False: quantize_mxfp4_rows(w), dequantize=dequantize_mxfp4_rows,
                       native_counter="mxfp4_native_calls", fallback_counter="mxfp4_fallback_calls")
WEIGHT_FORMATS = {f.weight_dtype: f for f in (_BF16, _FP8, _MXFP4)}


def weight_format(w, w_scale):
    """The record of a (w, w_scale) pair: uint8 weights are MXFP4 nibbles, any other weights with a scale are FP8, weights without
    one are bf16 (as it has been: a bf16 matrix WITH a scale is refused by the FP8 check, FP8 bytes WITHOUT one are not caught)."""
    if w.dtype == torch.uint8:
        return _MXFP4
    return _FP8 if w_scale is not None else _BF16


def _rows_modes_refuse(fp8_rows, mxfp4_rows):
    if fp8_rows not in FP8_ROWS_MODES:
        raise ValueError(f"fp8_rows must be one of {FP8_ROWS_MODES}, got {fp8_rows!r}")
    raise ValueError(f"mxfp4_rows must be one of {MXFP4_ROWS_MODES}, got {mxfp4_rows!r}")


def _linear_fallback(fmt, x, w, w_scale, bias, fuse_silu_mul, out):
    """F.linear.  A quantised format is CORRECT AND SLOW here: the weights are dequantised to a temporary of x's dtype on every
    call (counted).  What becomes of `out` differs and is carried as it has been: the quantised formats copy the result into it
    and return it, bf16 returns F.linear's own tensor and leaves `out` untouched."""
    if fmt.dequantize is None:
        y = F.linear(x, w, bias)
        return silu_and_mul_fused(y) if fuse_silu_mul else y
    globals()[fmt.fallback_counter] += 1
    y = F.linear(x, fmt.dequantize(w, w_scale, x.dtype), bias)
    if fuse_silu_mul:
        y = silu_and_mul_fused(y)
    return y if out is None else out.copy_(y)


def linear_decode(x, w, bias=None, fuse_silu_mul=False, out=None, near_pull=None, w_scale=None, fp8_rows="fallback",
                  mxfp4_rows="fallback"):
    """F.linear for decode-time activations (x [..., K] with a handful of token rows).  fuse_silu_mul: w = [gate; up] ->
    silu(gate.x) * (up.x).  out: a caller-owned result buffer.  The weight format follows from (w, w_scale) - weight_format();
    for every format, in this order:
      near_pull (the down projection of a ShadowKV layer; ShadowKVCache_CPU.near_pull_args(layer, 1)): one native token row with
        N <= 8192 and no fused SiLU, else ValueError; the GEMV launch's first workgroups stage the second near-miss list of this
        step's selection (skv_gemv_near_pull_<format>); same y.
      2..MAX_GEMV_ROWS native token rows -> the small-M MFMA kernel (skv_linear_rows_<format>): the weights stream once.
      anything else but one native token row -> F.linear, over dequantised weights where the format is quantised (correct, slow).
      one native token row -> the GEMV (skv_gemv_<format>).
    Native means contiguous x and w and a K the format's kernels take:
      format  w, w_scale                                          one row            2..32 rows                        counted
      bf16    bf16 [N, K], None                                   K % 32, K >= 512   the same                          no
      FP8     float8_e4m3fn [N, K], f32 [N] (quantize_fp8_rows)   K % 16, K >= 1024  fp8_rows="native", K % 64         fp8_*_calls
      MXFP4   uint8 [N, K / 2], uint8 [N, K / 32], contiguous     K % 32, K >= 1024  mxfp4_rows="native", K % 128,     mxfp4_*_calls
              (quantize_mxfp4_rows)                                                  x on the GPU
    fp8_rows / mxfp4_rows ("fallback" | "native") are checked on every call and read by their own format only (DESIGN.md
    sections 10, 10.1, 12, 12.1)."""
    if fp8_rows not in FP8_ROWS_MODES or mxfp4_rows not in MXFP4_ROWS_MODES:
        _rows_modes_refuse(fp8_rows, mxfp4_rows)
    K = x.shape[-1]
    rows = x.numel() // K
    fmt = _MXFP4 if w.dtype == torch.uint8 else _FP8 if w_scale is not None else _BF16         # weight_format(w, w_scale)
    if fmt.validate is not None:
        fmt.validate(x, w, w_scale)
    N = w.shape[0]
    contiguous = x.is_contiguous() and w.is_contiguous() and (not fmt.scale_contiguous or w_scale.is_contiguous())
    one_row = rows == 1 and contiguous and K % fmt.k_step == 0 and K >= fmt.k_min
    if near_pull is not None:
        if not one_row or fuse_silu_mul or N > 8192:
            raise ValueError("near_pull rides in a one-token GEMV launch with at most 8,192 output rows")
        symbol, tail = fmt.gemv_near_pull, (N, K) + tuple(near_pull)
    elif 2 <= rows <= MAX_GEMV_ROWS and contiguous and K % fmt.rows_k_step == 0 and K >= fmt.rows_k_min \
            and (fmt.rows_keyword is None or (fp8_rows if fmt.rows_keyword == "fp8_rows" else mxfp4_rows) == "native") \
            and (x.is_cuda or not fmt.rows_gpu):
        symbol, tail = fmt.linear_rows, (rows, N, K, 1 if fuse_silu_mul else 0)
    elif not one_row:
        return _linear_fallback(fmt, x, w, w_scale, bias, fuse_silu_mul, out)
    else:
        symbol, tail = fmt.gemv, (N, K, 1 if fuse_silu_mul else 0)
    y = out if out is not None else torch.empty(x.shape[:-1] + ((N // 2) if fuse_silu_mul else N,), dtype=x.dtype, device=x.device)
    head = (ptr(w), ptr(w_scale)) if fmt.scaled else (ptr(w),)
    rc = getattr(lib(), symbol)(*head, ptr(x), ptr(bias), ptr(y), *tail, current_stream_handle())
    if rc:
        check(rc, fmt.what[symbol])
    if fmt.scaled:
        globals()[fmt.native_counter] += 1
    return y


def range_max_supported(x_numel, K, N):
    """Whether norm_linear_decode(..., range_max=) takes the one-launch path that fills the sampler's range keys."""
    return x_numel == K == 4096 and N % 16 == 0 and N // 16 <= 16384


def norm_linear_decode(x, residual, norm_w, eps, w, bias=None, fuse_silu_mul=False, out=None, h_out=None, range_max=None,
                       near_pull=None, w_scale=None, fp8_rows="fallback", mxfp4_rows="fallback"):
    """(h, y): h = x + residual (residual None -> h = x), y = linear(RMSNorm(h) * norm_w).  One token with hidden size 4096 and
    contiguous operands (x, w; MXFP4: and w_scale) is one native launch, skv_norm_gemv_<format> (the same h, bit for bit, in every
    format); anything else is add_rmsnorm + linear_decode(..., w_scale=, fp8_rows=, mxfp4_rows=) - formats and keywords as in
    linear_decode.  out / h_out: caller-owned result buffers (the eager decode paths reuse theirs instead of allocating per call).
    Two roles ride in the one launch only - ValueError elsewhere:
      near_pull (gate/up launch of a ShadowKV layer: fused SiLU, no bias, no range_max; ShadowKVCache_CPU.near_pull_args(layer)):
        the launch's first workgroups stage the near misses of this step's selection ahead of the next step
        (skv_norm_gemv_near_pull_<format>); same y.
      range_max (lm_head: no fused SiLU; int16 [>= N // 16], 16-B aligned; range_max_supported(...) must hold): the launch also
        leaves the largest of every 16 outputs as the sampler's 16-bit key (sample_token_native(..., range_max=))."""
    if fp8_rows not in FP8_ROWS_MODES or mxfp4_rows not in MXFP4_ROWS_MODES:
        _rows_modes_refuse(fp8_rows, mxfp4_rows)
    K = x.shape[-1]
    fmt = _MXFP4 if w.dtype == torch.uint8 else _FP8 if w_scale is not None else _BF16         # weight_format(w, w_scale)
    if fmt.validate is not None:
        fmt.validate(x, w, w_scale)
    N = w.shape[0]
    one_launch = x.numel() == K == 4096 and x.is_contiguous() and w.is_contiguous() \
        and (not fmt.scale_contiguous or w_scale.is_contiguous())
    if near_pull is not None and (not one_launch or not fuse_silu_mul or bias is not None or range_max is not None):
        raise ValueError("near_pull rides in the one-token gate/up launch (hidden size 4096, fused SiLU * mul, no bias)")
    if range_max is not None and (not one_launch or fuse_silu_mul or not range_max_supported(x.numel(), K, N)):
        raise ValueError("range_max: one token, hidden size 4096, N % 16 == 0, N <= 262,144, no fused SiLU")
    if not one_launch:
        h, hs = add_rmsnorm(x, residual, norm_w, eps)
        return h, linear_decode(hs, w, bias, fuse_silu_mul, out=out, w_scale=w_scale, fp8_rows=fp8_rows, mxfp4_rows=mxfp4_rows)
    y = out if out is not None else torch.empty(x.shape[:-1] + ((N // 2) if fuse_silu_mul else N,), dtype=x.dtype, device=x.device)
    h = (h_out if h_out is not None else torch.empty_like(x)) if residual is not None else x
    if near_pull is not None:
        symbol, tail = fmt.norm_gemv_near_pull, (ptr(y), N, K) + tuple(near_pull)
    elif range_max is not None:
        symbol, tail = fmt.norm_gemv_rangemax, (ptr(bias), ptr(y), N, K, ptr(range_max))
    else:
        symbol, tail = fmt.norm_gemv, (ptr(bias), ptr(y), N, K, 1 if fuse_silu_mul else 0)
    head = (ptr(w), ptr(w_scale)) if fmt.scaled else (ptr(w),)
    rc = getattr(lib(), symbol)(*head, ptr(x), ptr(residual), ptr(norm_w), float(eps), ptr(h) if residual is not None else 0, *tail,
                                current_stream_handle())
    if rc:
        check(rc, fmt.what[symbol])
    if fmt.scaled:
        globals()[fmt.native_counter] += 1
    return h, y


def add_rmsnorm(x, residual, w, eps):
    """(h, y): h = x + residual (bf16; residual None -> h = x), y = RMSNorm(h) * w.  One native launch."""
    shape = x.shape
    x2 = x.reshape(-1, shape[-1])
    h = torch.empty_like(x2) if residual is not None else x2
    y = torch.empty_like(x2)
    check(lib().skv_add_rmsnorm(ptr(x2), ptr(residual.reshape(-1, shape[-1]) if residual is not None else None),
                                ptr(w), ptr(h) if residual is not None else 0, ptr(y), x2.shape[0], shape[-1],
                                float(eps), current_stream_handle()), "add_rmsnorm")
    return h.view(shape), y.view(shape)


def silu_and_mul_fused(x):
    """silu(x[..., :d]) * x[..., d:] in one native launch (x contiguous)."""
    d = x.shape[-1] // 2
    out = torch.empty(x.shape[:-1] + (d,), dtype=x.dtype, device=x.device)
    check(lib().skv_silu_and_mul(ptr(x), ptr(out), x.numel() // x.shape[-1], d, current_stream_handle()),
          "silu_and_mul")
    return out


def qkv_rope_update(qkv, cos_sin, pos, row_idx, k_cache, v_cache, q_heads, kv_heads, q_override=None, q_out=None):
    """qkv [bs, 1, (Hq+2Hkv)*D] -> q [bs, Hq, 1, D] rotated at pos [bs] (int64, device); k (rotated) and v are
    written into row row_idx[0] (int64, device) of k_cache / v_cache [bs, Hkv, rows, D].  One native launch."""
    bs = qkv.shape[0]
    D = k_cache.shape[-1]
    width = cos_sin.shape[-1]
    q = q_out if q_out is not None else torch.empty(bs, q_heads, 1, D, dtype=qkv.dtype, device=qkv.device)
    check(lib().skv_qkv_rope_update(ptr(qkv), ptr(cos_sin), ptr(pos), ptr(row_idx), ptr(q_override), ptr(q),
                                    ptr(k_cache), ptr(v_cache), bs, q_heads, kv_heads, D, cos_sin.stride(0),
                                    cos_sin.shape[0], k_cache.stride(0), k_cache.stride(1), k_cache.shape[2],
                                    1 if width == 128 else 2,
                                    current_stream_handle()), "qkv_rope_update")
    return q


def norm_qkv_rope_update(x, residual, norm_w, eps, wqkv, bqkv, cos_sin, pos, row_idx, k_cache, v_cache, q_heads,
                         kv_heads, q_override=None, w_scale=None, fp8_rows="fallback", mxfp4_rows="fallback"):
    """(h, q) for ONE token of ONE sequence: h = x + residual, q = RoPE(split(linear(RMSNorm(h)))) [1, Hq, 1, D];
    rotated k and v are pushed into row row_idx of k_cache / v_cache [1, Hkv, rows, D].  One native launch
    (skv_qkv_gemv_rope_update[_<format>]) when the hidden size is 4096, head_dim 128, bs == 1 and the operands are contiguous
    (x, wqkv; MXFP4: and w_scale); otherwise norm_linear_decode + qkv_rope_update.  Formats (wqkv, w_scale) and the rows keywords
    (the multi-row path's projection) as in linear_decode."""
    if fp8_rows not in FP8_ROWS_MODES or mxfp4_rows not in MXFP4_ROWS_MODES:
        _rows_modes_refuse(fp8_rows, mxfp4_rows)
    K = x.shape[-1]
    D = k_cache.shape[-1]
    fmt = _MXFP4 if wqkv.dtype == torch.uint8 else _FP8 if w_scale is not None else _BF16      # weight_format(wqkv, w_scale)
    if fmt.validate is not None:
        fmt.validate(x, wqkv, w_scale)
    if x.numel() != K or K != 4096 or not x.is_contiguous() or not wqkv.is_contiguous() or D != 128 \
            or (fmt.scale_contiguous and not w_scale.is_contiguous()):
        h, qkv = norm_linear_decode(x, residual, norm_w, eps, wqkv, bqkv, w_scale=w_scale, fp8_rows=fp8_rows, mxfp4_rows=mxfp4_rows)
        return h, qkv_rope_update(qkv, cos_sin, pos, row_idx, k_cache, v_cache, q_heads, kv_heads, q_override)
    q = torch.empty(1, q_heads, 1, D, dtype=x.dtype, device=x.device)
    h = torch.empty_like(x) if residual is not None else x
    head = (ptr(wqkv), ptr(w_scale)) if fmt.scaled else (ptr(wqkv),)
    rc = getattr(lib(), fmt.qkv_gemv_rope_update)(
        *head, ptr(x), ptr(residual), ptr(norm_w), float(eps), ptr(h) if residual is not None else 0, ptr(bqkv), ptr(cos_sin), ptr(pos),
        ptr(row_idx), ptr(q_override), ptr(q), ptr(k_cache), ptr(v_cache), K, q_heads, kv_heads, D, cos_sin.stride(0), cos_sin.shape[0],
        k_cache.stride(1), k_cache.shape[2], 1 if cos_sin.shape[-1] == 128 else 2, current_stream_handle())
    if rc:
        check(rc, fmt.what[fmt.qkv_gemv_rope_update])
    if fmt.scaled:
        globals()[fmt.native_counter] += 1
    return h, q


def kv_proj_split_supported(x, wqkv, k_cache):
    """Shapes norm_q_rope + the k/v role take: one token of one sequence, hidden size 4096, head_dim 128, bf16 weights (the
    k/v role reads bf16 rows: FP8 and MXFP4 models use the one QKV launch)."""
    K = x.shape[-1]
    return bool(wqkv.dtype == torch.bfloat16 and x.is_cuda and x.numel() == K == 4096 and x.is_contiguous() and wqkv.is_contiguous() and k_cache.shape[-1] == 128
                and k_cache.shape[0] == 1)


def norm_q_rope(x, residual, norm_w, eps, wqkv, bqkv, cos_sin, pos, row_idx, k_cache, v_cache, q_heads, kv_heads, q_override=None,
                placement=KV_PROJ_IN_TOPK):
    """(h, q, kv_proj): norm_qkv_rope_update over the q rows of wqkv alone - one native launch; the k / v rows (the new token's
    cache row) are left to a role of the layer's selection launches: hand kv_proj (a _lib.KvProjDesc) to
    ShadowKVCache_CPU.select_fetch_attend_inplace(..., kv_proj=).  The descriptor holds raw pointers: h, row_idx, pos and the
    other arguments must stay alive and unchanged until that call."""
    if wqkv.dtype == torch.float8_e4m3fn:
        raise ValueError("the q / kv split of the QKV projection reads bf16 weight rows: FP8 weights take norm_qkv_rope_update")
    if wqkv.dtype == torch.uint8:
        raise ValueError("the q / kv split of the QKV projection reads bf16 weight rows: MXFP4 weights take norm_qkv_rope_update")
    if not kv_proj_split_supported(x, wqkv, k_cache):
        raise ValueError("the q / kv split of the QKV projection takes one token of one sequence, hidden size 4096, head_dim 128")
    K, D = x.shape[-1], 128
    q = torch.empty(1, q_heads, 1, D, dtype=x.dtype, device=x.device)
    h = torch.empty_like(x) if residual is not None else x
    rope_mode = 1 if cos_sin.shape[-1] == 128 else 2
    check(lib().skv_q_gemv_rope(ptr(wqkv), ptr(x), ptr(residual), ptr(norm_w), float(eps), ptr(h) if residual is not None else 0,
                                ptr(bqkv), ptr(cos_sin), ptr(pos), ptr(q_override), ptr(q), K, q_heads, kv_heads, D,
                                cos_sin.stride(0), cos_sin.shape[0], rope_mode, current_stream_handle()), "q_gemv_rope")
    desc = KvProjDesc(ptr(wqkv), ptr(h), ptr(norm_w), ptr(bqkv) or None, ptr(cos_sin), ptr(pos), ptr(row_idx), ptr(k_cache),
                      ptr(v_cache), cos_sin.stride(0), k_cache.stride(1), float(eps), K, q_heads, kv_heads, D, cos_sin.shape[0],
                      k_cache.shape[2], rope_mode, int(placement))
    return h, q, desc


# ---------------------------------------------------------------------------- RoPE (pure torch, tensor_op.py:127-151)
def rotate_half(x):
    half = x.shape[-1] // 2
    return torch.cat((-x[..., half:], x[..., :half]), dim=-1)


def apply_rotary_pos_emb(q, k, cos, sin, position_ids):
    cos = cos[position_ids].unsqueeze(1)
    sin = sin[position_ids].unsqueeze(1)
    return (q * cos) + (rotate_half(q) * sin), (k * cos) + (rotate_half(k) * sin)


def apply_rotary_pos_emb_single(q, cos, sin, position_ids, unsqueeze_dim=1):
    if position_ids.dim() == 3:  # [bs, heads, seq] -> one position per (b, h, s)
        flat = position_ids.reshape(-1, position_ids.size(-1))
        return (q * cos[flat]) + (rotate_half(q) * sin[flat])
    cos = cos[position_ids].unsqueeze(unsqueeze_dim)
    sin = sin[position_ids].unsqueeze(unsqueeze_dim)
    return (q * cos) + (rotate_half(q) * sin)


# ---------------------------------------------------------------------------- RoPE (native, tensor_op.py:154-238)
def apply_rotary_pos_emb_cuda(x, cos_sin, position_ids):
    bs, heads, seq_len, dim = x.shape
    out = torch.empty_like(x)
    shadowkv.apply_rotary_pos_emb_new(x, cos_sin, position_ids, out, bs, heads, seq_len, dim,
                                      x.stride(0), x.stride(1), x.stride(2), x.stride(3), cos_sin.stride(0),
                                      position_ids.stride(0), position_ids.stride(1), position_ids.stride(2),
                                      dim // 2)
    return out


def apply_rotary_pos_emb_cuda_push_cache(x, cos_sin, position_ids, chunk_size, cache, sparse_start, sparse_end, cnts):
    bs, heads, seq_len, dim = x.shape
    width = cos_sin.shape[-1]
    if width == 128:
        fn = shadowkv.apply_rotary_pos_emb_push_cache_opt
    elif width == 64:
        fn = shadowkv.apply_rotary_pos_emb_push_cache_opt_glm
    else:
        raise ValueError(f"Invalid cos_sin shape {cos_sin.shape}")
    fn(x, cos_sin, position_ids, cache, cnts, bs, heads, seq_len, dim,
       x.stride(0), x.stride(1), x.stride(2), x.stride(3), cos_sin.stride(0),
       position_ids.stride(0), position_ids.stride(1), position_ids.stride(2),
       cache.stride(0), cache.stride(1), cache.stride(2), int(sparse_start), int(sparse_end), dim // 2,
       int(chunk_size))
    return cache


def batch_gather_gemm_rotary_pos_emb_cuda(a, b, cos_sin, position_ids, output, chunk_size, cache, sparse_start,
                                          sparse_end, cnts):
    """Two-launch form with the reference's signature (gather-GEMM into `output`, then RoPE-and-push).
    The decode path of ShadowKVCache_CPU uses the fused single launch (`rebuild_keys`) instead."""
    bs, seq_len, rank = a.shape
    _, heads, head_dim, _ = b.shape
    max_seq_len = cos_sin.shape[0]
    num_chunks = position_ids.shape[-1]
    pid32 = position_ids.to(torch.int32).contiguous()
    shadowkv.batch_gather_gemm(a.contiguous(), b.contiguous(), cos_sin, cos_sin, pid32, output, bs, heads, seq_len,
                               head_dim, rank, num_chunks * chunk_size, max_seq_len, chunk_size, cnts)
    return apply_rotary_pos_emb_cuda_push_cache(output, cos_sin, pid32, chunk_size, cache, sparse_start, sparse_end,
                                                cnts)


def rebuild_keys(U, SV, cos_sin, position_ids, cnts, cache, sparse_start, chunk_size, hit_temp=None,
                 hit_offsets=None):
    """Fused K rebuild: cache[b,h,sparse_start+i] = RoPE(bf16(U[b,pos(i)].SV[b,h]^T)) for chunks >= cnts.
    U [bs, seq, r], SV [bs, heads, 128, r], position_ids int64 [bs, heads, S], cache [bs, heads, rows, 128]."""
    bs, seq_len, rank = U.shape
    heads, head_dim = SV.shape[1], SV.shape[2]
    width = cos_sin.shape[-1]
    if width not in (128, 64):
        raise ValueError(f"Invalid cos_sin shape {cos_sin.shape}")
    check(lib().skv_rebuild_keys(ptr(U), ptr(SV), ptr(cos_sin), ptr(position_ids), ptr(cnts), ptr(cache), bs, heads,
                                 seq_len, head_dim, rank, position_ids.shape[-1], int(chunk_size), cos_sin.stride(0),
                                 cache.stride(0), cache.stride(1), cache.stride(2), int(sparse_start),
                                 1 if width == 128 else 2, ptr(hit_temp), ptr(hit_offsets), current_stream_handle()),
          "rebuild_keys")
    return cache


# ---------------------------------------------------------------------------- attention
_attn_ws = {}


def attention_workspace(device, bs, Hq, splits):
    """Per (device, shape, stream) scratch for the split records of the attention kernels (streams may run
    concurrently, so they never share one)."""
    key = (device.index, bs, Hq, splits, current_stream_handle())
    ws = _attn_ws.get(key)
    if ws is None:
        ws = torch.empty(lib().skv_attn_workspace_bytes(bs, Hq, splits), dtype=torch.uint8, device=device)
        _attn_ws[key] = ws
    return ws


def default_attention_splits(bs, Hkv, rows):
    """Splits of the standalone attention pass when the caller names none: one workgroup per (kv head, split) to fill the
    256 CUs (profiles/r02_attn_mfma_probe.txt: 64 splits beat 32 for 4 KV heads), at most 60 (the combine kernel merges up
    to 62 records); long rows (full-attention baseline: 125 K keys per head) get a split per ~2 K keys whatever the batch,
    so that every CU holds several workgroups."""
    return max(1, min(60, max(256 // max(1, bs * Hkv), -(-rows // 2048))))


def sparse_attention_decode(q, k_cache, v_cache, kv_len=None, kv_len_dev=None, splits=None, out=None, slots=None,
                            select_sets=0, sparse_start=0, resident_sets=0):
    """softmax(q K^T / sqrt(D)) V for q_len == 1 over the first kv_len rows of the cache views.
    q [bs, Hq, 1, D] or [bs, Hq, D]; k_cache / v_cache [bs, Hkv, rows, D] views of contiguous
    [bs, Hkv, buf_rows, D] buffers (what get_key_cache / get_value_cache return).  Returns
    [bs, 1, Hq, D] like flash_attn_with_kvcache's output for q [bs, 1, Hq, D].
    slots (int32 [bs * Hkv, select_sets], with sparse_start / resident_sets): a resident set larger than the selection -
    of the rows [sparse_start, sparse_start + 8 * resident_sets) only the listed chunks are attended."""
    bs, Hq = q.shape[0], q.shape[1]
    D = q.shape[-1]
    Hkv = k_cache.shape[1]
    rows = k_cache.shape[2]
    if kv_len is None:
        kv_len = rows
    if kv_len_dev is None and not 1 <= int(kv_len) <= rows:
        raise ValueError(f"kv_len {kv_len} outside the {rows} rows of the cache view")
    if k_cache.stride(3) != 1 or k_cache.stride(2) != D or k_cache.stride(0) != Hkv * k_cache.stride(1) \
            or k_cache.stride() != v_cache.stride():
        raise ValueError("k/v cache views must be row-contiguous slices of [bs, Hkv, rows, D] buffers")
    if not q.is_contiguous():
        q = q.contiguous()
    if splits is None:
        splits = default_attention_splits(bs, Hkv, rows)
    ws = attention_workspace(q.device, bs, Hq, splits)
    if out is None:
        out = torch.empty(bs, 1, Hq, D, dtype=q.dtype, device=q.device)
    if slots is not None:
        check(lib().skv_sparse_attention_slots(ptr(q), ptr(k_cache), ptr(v_cache), ptr(out), ptr(ws), ptr(kv_len_dev),
                                               int(kv_len), rows, k_cache.stride(1), bs, Hq, Hkv, D, splits,
                                               1.0 / math.sqrt(D), ptr(slots), int(select_sets), int(sparse_start),
                                               int(resident_sets), current_stream_handle()), "sparse_attention_slots")
        return out
    check(lib().skv_sparse_attention(ptr(q), ptr(k_cache), ptr(v_cache), ptr(out), ptr(ws), ptr(kv_len_dev),
                                     int(kv_len), rows, k_cache.stride(1), bs, Hq, Hkv, D, splits, 1.0 / math.sqrt(D),
                                     current_stream_handle()), "sparse_attention")
    return out


def causal_attention_prefill(q, k, v, out=None):
    """Causal GQA attention over a prompt: flash_attn_with_kvcache(q, k, v, causal=True) at base.py:293 / :311, one native
    launch (skv_prefill_attention).  q [bs, Hq, S, D]; k / v [bs, Hkv, kv_len, D] views with kv_len >= S (any batch / head /
    row strides, last dimension contiguous: the transpose view of the fused QKV output, slices of the cache buffers).  Row i
    attends keys j <= kv_len - S + i (the mask aligned bottom-right).  Returns [bs, S, Hq, D] (flash-attn's layout: a
    reshape to [bs, S, Hq * D] is free).  bf16, D = 128."""
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise ValueError("q must be [bs, Hq, S, D], k / v [bs, Hkv, kv_len, D]")
    bs, Hq, S, D = q.shape
    Hkv, kv_len = k.shape[1], k.shape[2]
    if k.shape != v.shape or k.shape[0] != bs or k.shape[3] != D:
        raise ValueError(f"k {tuple(k.shape)} / v {tuple(v.shape)} do not match q {tuple(q.shape)}")
    if Hkv < 1 or Hq % Hkv:
        raise ValueError(f"{Hq} query heads are not a multiple of {Hkv} KV heads")
    if S < 1 or kv_len < S:
        raise ValueError(f"kv_len {kv_len} must be >= q_len {S} >= 1")
    if not (q.dtype == k.dtype == v.dtype == torch.bfloat16) or not (q.is_cuda and k.is_cuda and v.is_cuda):
        raise ValueError("q / k / v must be bf16 tensors on the GPU")

    def strides(t):             # (a size-1 dimension's stride is never followed: 0 keeps it out of the alignment check)
        return [st if n > 1 else 0 for n, st in zip(t.shape[:3], t.stride()[:3])]

    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.stride(3) != 1 or any(st % 8 for st in strides(t)) or t.data_ptr() % 16:
            raise ValueError(f"{name} must have a contiguous last dimension, strides that are multiples of 8 elements and a "
                             "16-byte aligned start")
    if out is None:
        out = torch.empty(bs, S, Hq, D, dtype=q.dtype, device=q.device)
    elif out.shape != (bs, S, Hq, D) or not out.is_contiguous() or out.dtype != q.dtype:
        raise ValueError("out must be a contiguous [bs, S, Hq, D] tensor of q's dtype")
    check(lib().skv_prefill_attention(ptr(q), ptr(k), ptr(v), ptr(out), bs, Hq, Hkv, S, kv_len, D, *strides(q), *strides(k),
                                      *strides(v), 1.0 / math.sqrt(D), current_stream_handle()), "prefill_attention")
    return out


def chunk_stats(k_ctx, chunk_size=8):
    """k_ctx bf16 [bs, kv, rows, D] (row-contiguous view, rows >= chunks*chunk_size used from row 0), D = 128 ->
    (means [bs, kv, chunks, D], min_cos [bs, kv, chunks]): kv_cache.py:854-868 in one native pass over K."""
    bs, kv, rows, D = k_ctx.shape
    if k_ctx.stride(3) != 1 or k_ctx.stride(2) != D or k_ctx.stride(0) != kv * k_ctx.stride(1):
        raise ValueError("k_ctx must be a row-contiguous [bs, kv, rows, D] view")
    chunks = rows // chunk_size
    means = torch.empty(bs, kv, chunks, D, dtype=k_ctx.dtype, device=k_ctx.device)
    min_cos = torch.empty(bs, kv, chunks, dtype=k_ctx.dtype, device=k_ctx.device)
    check(lib().skv_chunk_stats(ptr(k_ctx), k_ctx.stride(1), bs * kv, chunks, chunk_size, D, ptr(means), ptr(min_cos),
                                current_stream_handle()), "chunk_stats")
    return means, min_cos


# ---------------------------------------------------------------------------- MInference sparse prefill
MINFERENCE_TYPES = ("vertical_and_slash", "stream_llm")      # "block_sparse" is refused
VS_SINKS, VS_LOCAL = 30, 100          # columns / diagonal offsets the estimate always keeps
VS_MIN_VERTICAL, VS_MIN_SLASH = 30, 50
INDEX_PAD = 2 ** 31 - 1               # list padding: entries outside [0, L) are ignored by the kernel


def _check_prompt_qkv(q, k, v=None):
    if q.dim() != 4 or k.dim() != 4 or (v is not None and v.dim() != 4):
        raise ValueError("q must be [bs, Hq, L, D], k / v [bs, Hkv, L, D]")
    bs, Hq, L, D = q.shape
    Hkv = k.shape[1]
    if k.shape[0] != bs or k.shape[2] != L or k.shape[3] != D or (v is not None and v.shape != k.shape):
        raise ValueError(f"k {tuple(k.shape)} / v do not match q {tuple(q.shape)} (the sparse prefill needs kv_len == q_len)")
    if Hkv < 1 or Hq % Hkv:
        raise ValueError(f"{Hq} query heads are not a multiple of {Hkv} KV heads")
    ts = (q, k) if v is None else (q, k, v)
    if any(t.dtype != torch.bfloat16 or not t.is_cuda for t in ts):
        raise ValueError("q / k / v must be bf16 tensors on the GPU")
    for name, t in zip("qkv", ts):
        if t.stride(3) != 1 or any(st % 8 for st in _row_strides(t)) or t.data_ptr() % 16:
            raise ValueError(f"{name} must have a contiguous last dimension, strides that are multiples of 8 elements and a "
                             "16-byte aligned start")
    return bs, Hq, Hkv, L, D


def _row_strides(t):            # (a size-1 dimension's stride is never followed: 0 keeps it out of the alignment check)
    return [st if n > 1 else 0 for n, st in zip(t.shape[:3], t.stride()[:3])]


def vertical_slash_scores(q, k):
    """The vertical + slash estimate (tensor_op.py:86-101 of the reference, restated in DESIGN.md section 9), one native pair
    of launches for every (sequence, query head): from the last m = min(64, L) queries, A = q k^T WITHOUT the 1 / sqrt(D)
    scale, causal, P = softmax in f32; returns (c [bs, Hq, L], d [bs, Hq, L]) f32 with c[j] = sum_r P[r, j] (+inf for j < 30)
    and d[s] = sum_r P[r, r - s] (+inf for s < 100).  q [bs, Hq, L, D], k [bs, Hkv, L, D] views (last dimension contiguous).
    Deterministic: the same inputs give bit-identical scores."""
    bs, Hq, Hkv, L, D = _check_prompt_qkv(q, k)
    c = torch.empty(bs, Hq, L, dtype=torch.float32, device=q.device)
    d = torch.empty_like(c)
    ws = torch.empty(max(1, lib().skv_vs_estimate_workspace_bytes(bs, Hq, L)), dtype=torch.uint8, device=q.device)
    check(lib().skv_vs_estimate(ptr(q), ptr(k), ptr(c), ptr(d), ptr(ws), bs, Hq, Hkv, L, L, D, *_row_strides(q),
                                *_row_strides(k), current_stream_handle()), "vs_estimate")
    return c, d


def _per_head(x, Hq, what):
    if isinstance(x, int):
        return [x] * Hq
    x = [int(v) for v in x]
    if len(x) != Hq:
        raise ValueError(f"{what}: {len(x)} per-head sizes for {Hq} query heads")
    return x


def _top_sorted(score, counts):
    """score [bs, Hq, L]; counts: per-head list -> int32 [bs, Hq, max(counts)], each row the top counts[h] indices in
    ascending order, padded with INDEX_PAD (torch.topk, as the reference)."""
    kmax = max(counts)
    idx = torch.topk(score, kmax, dim=-1).indices.to(torch.int32)
    cnt = torch.tensor(counts, dtype=torch.int64, device=score.device).view(1, -1, 1)
    keep = torch.arange(kmax, device=score.device).view(1, 1, -1) < cnt
    idx = torch.where(keep, idx, torch.full_like(idx, INDEX_PAD))
    return torch.sort(idx, dim=-1).values


def vertical_slash_indices(q, k, vertical_size, slash_size, scores=None):
    """The "vertical_and_slash" index sets: (vertical_idx, slash_idx) int32 [bs, Hq, n], each row ascending and padded with
    INDEX_PAD.  Head h keeps the top min(L, max(vertical_size[h], 30)) columns by c and the top min(L, max(slash_size[h],
    50)) diagonal offsets by d (vertical_slash_scores; pass `scores` = (c, d) to reuse them).  vertical_size / slash_size:
    an int or one value per query head."""
    bs, Hq, L = q.shape[0], q.shape[1], q.shape[2]
    vs = [min(L, max(n, VS_MIN_VERTICAL)) for n in _per_head(vertical_size, Hq, "vertical_size")]
    ss = [min(L, max(n, VS_MIN_SLASH)) for n in _per_head(slash_size, Hq, "slash_size")]
    c, d = vertical_slash_scores(q, k) if scores is None else scores
    return _top_sorted(c, vs), _top_sorted(d, ss)


def _fixed_sets(counts, L, bs, device):
    """stream_llm: [bs, Hq, max(counts)] int32 rows 0 .. counts[h] - 1, INDEX_PAD behind (entries >= L are ignored)."""
    kmax = max(counts)
    ar = torch.arange(kmax, dtype=torch.int32, device=device).view(1, 1, -1)
    cnt = torch.tensor(counts, dtype=torch.int32, device=device).view(1, -1, 1)
    return torch.where(ar < cnt, ar, torch.full_like(ar, INDEX_PAD)).expand(bs, -1, -1).contiguous()


def _index_rows(idx, bs, Hq, device):
    if not torch.is_tensor(idx):
        idx = torch.tensor(idx, device=device)
    if idx.dim() == 2:
        idx = idx.unsqueeze(0).expand(bs, -1, -1)
    if idx.dim() != 3 or idx.shape[0] != bs or idx.shape[1] != Hq or idx.shape[2] < 1:
        raise ValueError(f"index lists must be [bs, Hq, n] or [Hq, n] with n >= 1, got {tuple(idx.shape)}")
    if idx.dtype not in (torch.int32, torch.int64) or idx.device != torch.device(device):
        raise ValueError("index lists must be int32 / int64 tensors on q's device")
    return idx


def sparse_prefill_attention(q, k, v, vertical_idx, slash_idx, out=None, sorted=False):
    """Vertical + slash sparse causal attention, two native launches for every (sequence, query head):
    row i (block b = i // 64, e = 64 (b + 1)) attends key j <= i iff j is a vertical column or lies in the window
    [max(e - s, 64) - 64, max(e - s, 64)) of a slash offset s < e; softmax(q.k / sqrt(D)) over those keys times V.
    q [bs, Hq, L, D], k / v [bs, Hkv, L, D] views; vertical_idx / slash_idx [bs, Hq, n] (or [Hq, n]) integer lists in any
    order, duplicates allowed, entries outside [0, L) ignored; sorted=True promises int32 rows already ascending.
    Returns [bs, L, Hq, D] (a reshape to [bs, L, Hq * D] is free).  bf16, D = 128."""
    bs, Hq, Hkv, L, D = _check_prompt_qkv(q, k, v)
    vi = _index_rows(vertical_idx, bs, Hq, q.device)
    si = _index_rows(slash_idx, bs, Hq, q.device)
    if not sorted:
        # int64 entries beyond int32 are outside [0, L) either way
        vi = torch.sort(vi.clamp(-1, INDEX_PAD).to(torch.int32), dim=-1).values
        si = torch.sort(si.clamp(-1, INDEX_PAD).to(torch.int32), dim=-1).values
    elif vi.dtype != torch.int32 or si.dtype != torch.int32:
        raise ValueError("sorted=True needs int32 index lists")
    vi, si = vi.contiguous(), si.contiguous()
    if out is None:
        out = torch.empty(bs, L, Hq, D, dtype=q.dtype, device=q.device)
    elif out.shape != (bs, L, Hq, D) or not out.is_contiguous() or out.dtype != q.dtype:
        raise ValueError("out must be a contiguous [bs, L, Hq, D] tensor of q's dtype")
    ws = torch.empty(max(1, lib().skv_vs_attention_workspace_bytes(bs, Hq, L)), dtype=torch.uint8, device=q.device)
    check(lib().skv_vs_sparse_attention(ptr(q), ptr(k), ptr(v), ptr(out), ptr(vi), ptr(si), ptr(ws), bs, Hq, Hkv, L, L, D,
                                        vi.shape[-1], si.shape[-1], *_row_strides(q), *_row_strides(k), *_row_strides(v),
                                        1.0 / math.sqrt(D), current_stream_handle()), "vs_sparse_attention")
    return out


def validate_minference_layer(pattern, Hq, where="pattern"):
    """{head: (type, vertical_size, slash_size, score)} -> the same dict with int heads and tuple values; ValueError for a
    head outside [0, Hq), an unknown or unsupported type, or a size that is not a positive integer."""
    if not isinstance(pattern, dict):
        raise ValueError(f"{where}: expected a dict {{head: [type, vertical_size, slash_size, score]}}")
    out = {}
    for head, entry in pattern.items():
        try:
            h = int(head)
        except (TypeError, ValueError):
            raise ValueError(f"{where}: head id {head!r} is not an integer") from None
        if not 0 <= h < Hq:
            raise ValueError(f"{where}, head {h}: head id outside [0, {Hq})")
        if not isinstance(entry, (list, tuple)) or len(entry) != 4:
            raise ValueError(f"{where}, head {h}: expected [type, vertical_size, slash_size, score], got {entry!r}")
        ty, vsz, ssz, score = entry
        if ty == "block_sparse":
            raise ValueError(f"{where}, head {h}: 'block_sparse' is not supported (DESIGN.md section 9)")
        if ty not in MINFERENCE_TYPES:
            raise ValueError(f"{where}, head {h}: unknown pattern type {ty!r}")
        for name, n in (("vertical_size", vsz), ("slash_size", ssz)):
            if isinstance(n, bool) or not isinstance(n, int) or n < 1:
                raise ValueError(f"{where}, head {h}: {name} must be a positive integer, got {n!r}")
        out[h] = (ty, vsz, ssz, score)
    return out


def minference_index_sets(query_states, key_states, minference_parttern):
    """The per-head (vertical_idx, slash_idx) lists of one layer (sorted int32, INDEX_PAD behind): "vertical_and_slash"
    heads from the estimate (one pair of launches for all heads, only when some head needs it), "stream_llm" heads the fixed
    sets {0 .. vertical_size - 1} and {0 .. slash_size - 1}."""
    bs, Hq, L = query_states.shape[0], query_states.shape[1], query_states.shape[2]
    pat = validate_minference_layer(minference_parttern, Hq)
    if len(pat) != Hq:
        raise ValueError(f"the layer pattern names {len(pat)} of {Hq} query heads")
    types = [pat[h][0] for h in range(Hq)]
    vsz = [pat[h][1] for h in range(Hq)]
    ssz = [pat[h][2] for h in range(Hq)]
    dev = query_states.device
    fixed_v, fixed_s = _fixed_sets(vsz, L, bs, dev), _fixed_sets(ssz, L, bs, dev)
    if all(t == "stream_llm" for t in types):
        return fixed_v, fixed_s
    est_v, est_s = vertical_slash_indices(query_states, key_states, vsz, ssz)
    stream = torch.tensor([t == "stream_llm" for t in types], device=dev).view(1, -1, 1)

    def pick(est, fixed):
        n = max(est.shape[-1], fixed.shape[-1])
        est = F.pad(est, (0, n - est.shape[-1]), value=INDEX_PAD)
        fixed = F.pad(fixed, (0, n - fixed.shape[-1]), value=INDEX_PAD)
        return torch.where(stream, fixed, est).contiguous()

    return pick(est_v, fixed_v), pick(est_s, fixed_s)


def minference_prefill_kernel(query_states, key_states, value_states, minference_parttern):
    """The reference's minference_prefill_kernel (tensor_op.py:68-117): q [bs, Hq, L, D], k / v [bs, Hkv, L, D] (kv_len ==
    q_len: a prompt), minference_parttern {head: (type, vertical_size, slash_size, score)} for every query head of the layer.
    Every head runs in the same launches (index estimate, then the sparse attention).  Returns [bs, L, Hq * D] contiguous."""
    bs, Hq, L, D = query_states.shape
    assert L > 1
    vi, si = minference_index_sets(query_states, key_states, minference_parttern)
    out = sparse_prefill_attention(query_states, key_states, value_states, vi, si, sorted=True)
    return out.view(bs, L, Hq * D)


# ---------------------------------------------------------------------------- sampling (tensor_op.py:242-297)
def top_k_top_p_filter(logits, top_k=0, top_p=0.0):
    if top_k > 0:
        kth = torch.topk(logits, min(top_k, logits.size(-1)))[0][:, [-1]]
        logits[logits < kth] = float("-inf")
    if top_p > 0.0:
        sorted_logits, sorted_idx = torch.sort(logits, descending=True)
        remove = torch.cumsum(F.softmax(sorted_logits, dim=-1), dim=-1) > top_p
        remove[..., 1:] = remove[..., :-1].clone()
        remove[..., 0] = 0
        logits[remove.scatter(1, sorted_idx, remove)] = float("-inf")
    return logits


def norm_logits(logits, temperature=0.6, top_k=-1, top_p=0.9):
    assert logits.dim() == 2
    if temperature != 1.0:
        logits = logits / temperature
    return F.softmax(top_k_top_p_filter(logits, top_k=top_k, top_p=top_p), dim=-1)


def sample(probs, num_samples=1):
    return torch.multinomial(probs, num_samples=num_samples, replacement=True)


_sampler_state = {}
_sampler_seed = None


def set_sampler_seed(seed):
    """Seed of the native sampler's counter-based random numbers (None: follow torch.initial_seed(), i.e. what
    torch.manual_seed(...) last set).  A new seed restarts every draw counter, so `manual_seed(s)` followed by the same calls
    draws the same tokens."""
    global _sampler_seed
    _sampler_seed = None if seed is None else int(seed)


def sample_token_native(logits, temperature, top_k, top_p, seed=None, state=None, range_max=None):
    """sample_token in ONE native launch for bf16 logits [bs, V] on the GPU (skv_sample_topk_advance: exact k-th value,
    every logit tied with it kept - the reference's filter -, logit / temperature, nucleus, draw).  Same distribution as
    the torch pipeline below; the random numbers are NOT torch's generator stream: they come from a counter-based hash of
    (seed, draw counter, row) with seed = `seed`, else set_sampler_seed(), else torch.initial_seed() (so torch.manual_seed
    reseeds it), and a draw counter kept per `state` (any dict a caller owns - one per model or generation - default: one
    per (device, batch size) of the process).  Returns None when the kernel does not take the row (caller falls back).
    range_max (int16 [bs, >= V // 16], from norm_linear_decode(..., range_max=) of the SAME logits): the sampler reads the
    keys and the ~k ranges that can hold a winner instead of the whole row - same token."""
    bs, V = logits.shape
    k = min(top_k, V) if top_k > 0 else V
    if not (logits.is_cuda and logits.dtype == torch.bfloat16 and temperature > 0.0 and 1 <= k <= 64 and V % 8 == 0
            and V <= 4 * 131072 and logits.stride(-1) == 1 and logits.stride(0) % 8 == 0 and logits.data_ptr() % 16 == 0):
        return None
    if seed is None:
        seed = _sampler_seed if _sampler_seed is not None else torch.initial_seed()
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (logits.device.index, bs)
    holder = _sampler_state if state is None else state
    st = holder.get(key)
    if st is None:
        dev = logits.device
        st = dict(pos=torch.zeros(bs, 1, dtype=torch.long, device=dev), gen=torch.zeros(1, dtype=torch.long, device=dev),
                  row=torch.zeros(1, dtype=torch.long, device=dev), kvl=torch.zeros(1, dtype=torch.int32, device=dev),
                  seed=seed)
        holder[key] = st
    elif st["seed"] != seed:            # reseeded: the draw counter starts again
        st["gen"].zero_()
        st["pos"].zero_()
        st["seed"] = seed
    token = torch.empty(bs, 1, dtype=torch.long, device=logits.device)
    if range_max is not None and V % 16 == 0 and V // 16 <= 16384 and V // 16 >= k:
        rm = range_max.view(bs, -1)
        check(lib().skv_sample_topk_advance_ranges(ptr(logits), logits.stride(0), V, ptr(rm), rm.stride(0), bs, k, float(temperature),
                                                   float(top_p), seed, ptr(token), ptr(st["pos"]), ptr(st["gen"]), ptr(st["row"]),
                                                   ptr(st["kvl"]), 0, 0, 1, 1, 0, 0, 0, current_stream_handle()),
              "sample_topk_advance_ranges")
        return token
    check(lib().skv_sample_topk_advance(ptr(logits), logits.stride(0), V, bs, k, float(temperature), float(top_p), seed,
                                        ptr(token), ptr(st["pos"]), ptr(st["gen"]), ptr(st["row"]), ptr(st["kvl"]), 0, 0, 1, 1,
                                        0, 0, 0, current_stream_handle()), "sample_topk_advance")
    return token


def sample_token(logits, temperature=0, top_k=50, top_p=0.9, state=None, range_max=None):
    """tensor_op.py:291-297.  bf16 logits on the GPU take the native sampler, whose random numbers are not torch's generator
    stream (see sample_token_native: seeded from torch.initial_seed() / set_sampler_seed, draw counter per `state`)."""
    if temperature == 0.0:
        return logits.argmax(dim=-1, keepdim=True)
    if logits.dtype == torch.bfloat16 and logits.is_cuda:     # the lm_head's own output: one native launch
        tok = sample_token_native(logits, temperature, top_k, top_p, state=state, range_max=range_max)
        if tok is not None:
            return tok
        logits = logits.float()
    return sample(norm_logits(logits, temperature=temperature, top_p=top_p, top_k=top_k))
