"""`ShadowKVCache_CPU` for MI355X: same constructor, methods, attributes and buffer layout as the
reference's offload cache (/root/reference/models/kv_cache.py:509-1319) so the reference's host
models (`LLM.layer_compute`, models/base.py:296-341) can drive it unchanged; the decode-time
methods launch the hand-written gfx950 kernels of libshadowkv_hip.so.

State (per layer l, batch b, KV head h; D = head_dim, C = chunk_size, S = sparse_budget // C):
  v_cache_cpu   pinned host  [L, bs, kv, max_length // C, C*D]   every V chunk, 2 KiB rows (C=8, D=128)
        v_dtype="fp8_e4m3": float8_e4m3fn, 1 KiB rows, + v_scale f32 [L, bs, kv, max_length // C, C] in HBM
  k_/v_cache_buffer  HBM     [L, bs, kv, buf_len, D],  buf_len = R*C + 128 + (outlier + local)*C
        rows [0, prefill_local)            last tokens of the prompt (exact K / V)
        rows [prefill_local, sparse_start) outlier chunks (exact K / V)
        rows [sparse_start, sparse_end)    R chunk slots; slot i holds chunk position_ids[l,b,h,i] (R = S: the S selected
                                           chunks, the reference's layout; resident_sets = R > S: see __init__)
        rows [sparse_end, buf_len)         tokens generated so far
  U [L, bs, seq, r], SV [L, bs, kv, D, r]   rank-r factorisation of the pre-RoPE keys (r-contiguous)
  k_landmark [L, bs, kv, N, D], k_landmark_idx int64 [L, bs, kv, N]   chunk means + their chunk ids
        landmark_dtype="fp8_e4m3": float8_e4m3fn, 128-byte rows, + k_landmark_scale f32 [L, bs, kv, N]
  position_ids int64 [L, bs, kv, R], offsets int32 [bs*kv*S], cnts int32 [bs*kv], signals int32 [bs*kv]

MI355X-first differences that do not change results:
  * U / SV / landmarks are created in HBM straight away (288 GB): H2D() only sizes the decode
    workspaces; the reference parks them on the CPU until H2D() (kv_cache.py:694-696, :1178-1225).
  * get_retrieval_position_ids is ONE native call (score + softmax + group max + top-k + diff,
    no [bs,kv,G,N] round trips through torch.max / torch.topk / gather) followed by the staging launch
    of the chunk movement; get_key_cache is one fused landing + rebuild-RoPE-store launch (no `output`
    round trip); get_value_cache is one landing + PCIe-fetch launch.  No kernel spins on another.
  * the host V stride passed to the mover is the tensor's real stride (max_length // C chunks); the
    reference passes the prompt length (kv_cache.py:1090), identical whenever prompt == max_length.
  * top-k membership under exact bf16 ties is defined (lowest landmark slot); torch.topk's is not.

Beyond the reference's surface (opt-in, used by DecoderLM.forward_fused / bench.py):
  * select_fetch_inplace / select_fetch_attend_inplace: the same decode step with an in-place resident set (chunks
    selected again keep their slot, misses take the freed slots) and, optionally, the attention over the resident rows
    inside the PCIe-bound fetch launch - same chunk set, K / V bytes and attention values (up to summation order).
  * resident_sets > select_sets: more chunk slots stay resident than are attended (least-recently-selected
    replacement, in-place layout only) - same selections and outputs, fewer chunks over PCIe.
  * v_offload=False keeps the chunked V table in HBM; svd_mode="gram" factorises through K^T K;
    prefill_kv_cache computes chunk means / outlier scores in one native pass when the keys are on the GPU.
"""
import ctypes
import gc
import math
import weakref

import torch

from . import tensor_op
from ._lib import lib, check, ptr, current_stream_handle
from .kernels import shadowkv


def pinned_host_tensor(shape, dtype):
    """Exact-size page-locked, device-mapped host tensor (skv_host_alloc = hipHostMalloc in the HIP runtime torch itself
    uses: libshadowkv_hip.so is loaded after torch and resolves to the runtime already in the process) for the chunked V
    table.  torch's caching pinned allocator rounds every request up to a power of two (8.19 GB -> 16 GiB per 122K-token
    sequence; the reference's batch of 24 sequences, 197 GB, would ask for 256 GiB); the V table is allocated once and lives
    as long as the cache, so it bypasses that allocator.  The memory is owned by the buffer object every view of the tensor
    keeps alive: it is freed when the LAST view (slices such as v_cache_cpu[l] included) is gone, not when the cache is.
    torch recognises the memory as pinned (is_pinned()), so GPU -> host copies into it are asynchronous DMA."""
    as_bytes = dtype == torch.float8_e4m3fn          # (the buffer protocol has no float8: bytes, viewed as float8)
    nbytes = math.prod(shape) * (1 if as_bytes else torch.empty((), dtype=dtype).element_size())
    p = ctypes.c_void_p()
    rc = lib().skv_host_alloc(ctypes.byref(p), nbytes)
    if rc != 0 or not p.value:
        raise MemoryError(f"skv_host_alloc({nbytes} bytes of pinned host memory) failed: {lib().skv_last_error().decode()}")
    buf = (ctypes.c_char * nbytes).from_address(p.value)
    fin = weakref.finalize(buf, lib().skv_host_free, p.value)
    fin.atexit = False      # at interpreter exit the HIP runtime may already be gone: the OS reclaims the pages
    if as_bytes:
        return torch.frombuffer(buf, dtype=torch.uint8).view(dtype).view(shape)
    return torch.frombuffer(buf, dtype=dtype).view(shape)


class KV_Cache:
    """Full-attention KV cache (the baseline `attn_mode='full'` of the reference, kv_cache.py:32-153): same
    constructor and methods; K / V live in HBM from the start (the reference keeps them on the CPU until H2D())."""

    def __init__(self, config, batch_size=1, max_length=32 * 1024, device="cuda:0", dtype=torch.bfloat16):
        self.config = config
        self.max_length = max_length
        self.device = torch.device(device)
        self.dtype = dtype
        kv, D = config.num_key_value_heads, config.hidden_size // config.num_attention_heads
        self.k_cache = torch.zeros(config.num_hidden_layers, batch_size, kv, max_length, D, device=self.device, dtype=dtype)
        self.v_cache = torch.zeros(config.num_hidden_layers, batch_size, kv, max_length, D, device=self.device, dtype=dtype)
        self.num_layers = config.num_hidden_layers
        self.kv_offset = 0
        self.prefilled_batch = 0
        self.batch_size = batch_size

    def update_kv_cache(self, new_k_cache, new_v_cache, layer_idx):
        bsz, _, incoming, _ = new_v_cache.shape
        if bsz == self.batch_size:
            self.prefilled_batch = 0
        b0, lo = self.prefilled_batch, self.kv_offset
        self.k_cache[layer_idx][b0:b0 + bsz, :, lo:lo + incoming].copy_(new_k_cache)
        self.v_cache[layer_idx][b0:b0 + bsz, :, lo:lo + incoming].copy_(new_v_cache)
        key = self.k_cache[layer_idx][b0:b0 + bsz, :, :lo + incoming]
        value = self.v_cache[layer_idx][b0:b0 + bsz, :, :lo + incoming]
        if layer_idx == self.num_layers - 1:
            self.prefilled_batch += bsz
            if self.prefilled_batch == self.batch_size:
                self.kv_offset += incoming
        return key, value

    def note_kv_appended(self, incoming=1):
        self.kv_offset += incoming

    def print_stats(self):
        print(f"KVCache | max_length {self.max_length} | dtype {self.dtype} | cached {self.kv_offset}")

    def H2D(self):
        gc.collect()

    def clear(self):
        self.k_cache.zero_()
        self.v_cache.zero_()
        self.kv_offset = 0
        self.prefilled_batch = 0

    def get_kv_len(self):
        return self.kv_offset


def gram_factorize(k, rank):
    """Rank-`rank` factors of k [bs, L, H] (f32, L >> H) without a full SVD: the right
    singular vectors are the eigenvectors of the H x H Gram matrix K^T K (one tall-skinny GEMM; squaring the condition
    number only hurts the small singular values, the leading `rank` pairs kept here are the well-conditioned ones), so
        K^T K = V diag(s^2) V^T,   U_r = K V_r diag(1/s_r),   SV = diag(s_r) V_r^T,   U_r SV = K V_r V_r^T
    which is the same best rank-r approximation torch.svd gives (columns may differ by sign, the product does not).
    Two GEMMs of L x H x H / L x H x r and an H x H eigh instead of rocSOLVER's gesvd over the L x H matrix.
    Returns (U_r [bs, L, rank], SV [bs, rank, H]) in f32."""
    g = torch.matmul(k.transpose(1, 2), k)                                  # [bs, H, H]
    lam, vec = torch.linalg.eigh(g)                                         # ascending
    lam_r = lam[:, -rank:].flip(-1).clamp_min(0)
    v_r = vec[:, :, -rank:].flip(-1)                                        # [bs, H, rank], descending s
    s_r = lam_r.sqrt()
    # directions whose singular value is numerically zero (K of rank < `rank`, or below the f32 resolution of the Gram
    # matrix: eigenvalues are accurate to ~eps * lambda_max, i.e. singular values to ~sqrt(eps) * s_max) carry nothing but
    # rounding noise: their U column is set to 0 instead of noise / ~0 (the matching SV row is ~0 either way), so the
    # product stays the best approximation of the given rank and never holds inf / NaN
    keep = s_r > s_r[:, :1] * (torch.finfo(torch.float32).eps ** 0.5) * 4
    inv = torch.where(keep, 1.0 / s_r.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(s_r))
    u_r = torch.matmul(k, v_r) * inv.unsqueeze(1)
    return u_r, v_r.transpose(1, 2) * (s_r * keep).unsqueeze(-1)


class ShadowKVCache_CPU:
    def __init__(self, config, batch_size=1, max_length=32 * 1024, device="cuda:0", dtype=torch.bfloat16,
                 sparse_budget=2048, chunk_size=8, rank=160, svd_mode="auto", v_offload=True, resident_sets=None,
                 v_dtype="bf16", landmark_dtype="bf16"):
        if dtype != torch.bfloat16:
            raise ValueError("ShadowKVCache_CPU supports bfloat16 only (as the reference's kernels do)")
        if v_dtype not in tensor_op.V_DTYPES:           # (before anything is allocated)
            raise ValueError(f"v_dtype must be one of {tensor_op.V_DTYPES}, got {v_dtype!r}")
        if landmark_dtype not in tensor_op.LANDMARK_DTYPES:
            raise ValueError(f"landmark_dtype must be one of {tensor_op.LANDMARK_DTYPES}, got {landmark_dtype!r}")
        # "fp8_e4m3" (DESIGN.md section 13): k_landmark holds e4m3 bytes with one f32 power-of-two scale per landmark row
        # (k_landmark_scale, the V table's quantisation rule) - half the bytes of the decode scan, the one HBM-bound kernel of the
        # path.  Only the landmark table is quantised; the selection is the exact selection over the rounded landmarks.
        self.landmark_dtype = landmark_dtype
        self.k_landmark_scale = None
        # "fp8_e4m3" (DESIGN.md section 11): the chunked V table holds e4m3 bytes (1 KiB rows) with one f32 power-of-two scale
        # per token row in HBM (v_scale) - half the PCIe bytes per miss and half the pinned memory.  Only the table is
        # quantised; every V row of the sparse region equals dequant(table row of the chunk in that slot) at all times.
        self.v_dtype = v_dtype
        self.config = config
        self.batch_size = batch_size
        self.max_length = max_length
        self.device = torch.device(device)
        self.dtype = dtype
        self.num_attention_heads = config.num_attention_heads
        self.num_key_value_heads = config.num_key_value_heads
        self.num_key_value_groups = config.num_attention_heads // config.num_key_value_heads
        self.head_dim = config.hidden_size // config.num_attention_heads
        self.num_layers = config.num_hidden_layers

        self.sparse_budget = int(sparse_budget)
        self.chunk_size = chunk_size
        self.rank = rank
        # "auto" (default since round 4): the Gram factorisation when the keys are on a GPU (21.6 ms instead of torch.svd's
        # 2.1 s per layer at 122K: 0.7 s instead of 68 s per prefill), torch.svd on the CPU (the golden fixtures pin that path
        # to the reference bit for bit).  SURVEY.md 8c's criterion for this stage is the RECONSTRUCTION U.SV at rtol 1e-2 (an
        # SVD's signs / rotations are not unique), which tests/test_gpu_build.py asserts for the Gram path against the
        # reference-pinned factors and against torch.svd at the headline length.  "svd" keeps the reference's call everywhere.
        if svd_mode is None:
            svd_mode = "auto"
        if svd_mode not in ("auto", "svd", "gram"):
            raise ValueError("svd_mode must be 'auto' (Gram on a GPU, torch.svd on the CPU), 'svd' (torch.svd, the reference's "
                             "call) or 'gram' (K^T K eigendecomposition)")
        self.svd_mode = svd_mode
        self.local_chunk = 4
        self.outlier_chunk = int((self.sparse_budget // 1024) * 24)
        self.select_sets = self.sparse_budget // self.chunk_size
        assert self.select_sets * self.chunk_size == self.sparse_budget, \
            f"({self.select_sets}) * {self.chunk_size} != {self.sparse_budget}"
        # Resident set larger than the selection (in-place layout only; not in the reference, whose resident set IS the
        # last selection): `resident_sets` slots per head stay in HBM, a selected chunk found in any of them is a hit,
        # the misses replace the least recently selected slots.  Attention still covers exactly the `select_sets`
        # selected chunks - same outputs, fewer chunks over PCIe (HBM is plentiful on MI355X, the link is the roof).
        self.resident_sets = self.select_sets if resident_sets is None else int(resident_sets)
        if not self.select_sets <= self.resident_sets <= 1024:
            raise ValueError(f"resident_sets must be in [select_sets = {self.select_sets}, 1024]")
        self.resident_budget = self.resident_sets * self.chunk_size

        L, bs, kv, D, C = self.num_layers, batch_size, self.num_key_value_heads, self.head_dim, chunk_size
        on_gpu = self.device.type == "cuda"
        # the chunked V table: pinned host memory (the reference's offload, read over PCIe by the fetch kernel) or,
        # with v_offload=False, HBM (what the reference's GPU-resident ShadowKVCache does, kv_cache.py:155-506: the
        # same kernels then gather the misses at HBM speed; 8 GB per 122K-token sequence of the 288 GB)
        self.v_offload = bool(v_offload) or not on_gpu
        fp8_v = v_dtype == "fp8_e4m3"
        if fp8_v and (C != 8 or D != 128):
            raise ValueError("v_dtype='fp8_e4m3' is built for chunk_size 8 and head_dim 128 (1 KiB table rows)")
        table_shape, table_dtype = (L, bs, kv, max_length // C, D * C), (torch.float8_e4m3fn if fp8_v else dtype)
        if self.v_offload and on_gpu:
            self.v_cache_cpu = pinned_host_tensor(table_shape, table_dtype)
            (self.v_cache_cpu.view(torch.uint8) if fp8_v else self.v_cache_cpu).zero_()
        else:
            table = torch.zeros(table_shape, device=self.device if on_gpu else "cpu", dtype=torch.uint8 if fp8_v else dtype)
            self.v_cache_cpu = table.view(table_dtype) if fp8_v else table
        # one scale per token row of the FP8 table; always on `device` (the scales never cross the host link)
        self.v_scale = torch.ones(L, bs, kv, max_length // C, C, device=self.device, dtype=torch.float32) if fp8_v else None
        buf_len = self.resident_budget + 128 + (self.outlier_chunk + self.local_chunk) * C
        self.k_cache_buffer = torch.zeros(L, bs, kv, buf_len, D, device=self.device, dtype=dtype)
        self.v_cache_buffer = torch.zeros(L, bs, kv, buf_len, D, device=self.device, dtype=dtype)

        self.kv_offset = 0
        self.prefill = 0
        self.gen_offset = 0
        self.prefilled_batch = 0
        self.k_landmark = None
        self.k_landmark_idx = None
        self.U = None
        self.SV = None

        self.block_num = bs * kv
        self.offsets = torch.zeros(self.block_num * self.select_sets, device=self.device, dtype=torch.int32)
        # hit counts: one row per layer (a decode step leaves every layer's counts behind: statistics, and the captured
        # step can sum them in its last kernel); `cnts` - the reference's attribute - is the row of the layer being processed
        self._cnts_layers = torch.zeros(L, self.block_num, device=self.device, dtype=torch.int32)
        self.cnts = self._cnts_layers[0]
        self.signals = torch.zeros(self.block_num, device=self.device, dtype=torch.int32)   # reference attribute; unused
        self.position_ids = torch.full((L, bs, kv, self.resident_sets), -1, device=self.device, dtype=torch.int64)
        # steps since the chunk in a slot was last selected (maintained by the selection kernel when resident_sets >
        # select_sets; empty slots - position id -1 - count as oldest whatever is stored here)
        self._slot_age = torch.zeros(L, self.block_num, self.resident_sets, device=self.device, dtype=torch.int32)
        self._select_ws = None
        # staging buffers of the two-phase (spin-free) chunk movement: moved hit chunks of one layer.  `temp` is the
        # reference's attribute of the same shape (kv_cache.py:612-620) and IS the V staging buffer; `output` is the
        # pre-RoPE K scratch of the reference's two-launch key path (kv_cache.py:637-645), unused by the fused path.
        self._temp_k = torch.zeros(self.block_num, self.select_sets, C * D, device=self.device, dtype=dtype)
        self._temp_v = torch.zeros(self.block_num, self.select_sets, C * D, device=self.device, dtype=dtype)
        self.temp = self._temp_v.view(bs, kv, self.select_sets, C * D)
        self.output = torch.zeros(bs, kv, self.sparse_budget, D, device=self.device, dtype=dtype)
        self._staged_layer = -1
        self._dst_slots = None           # in-place layout: destination slot per miss (select_fetch_inplace)
        self._early = None               # speculative early V fetch (enable_early_fetch): per-layer states
        self._early_request = None       # (early_max, margin) to re-enable with after clear() + a new prefill (H2D)
        # Fused selection (round 4, csrc/skv_select.hip t3_fused_front): scan -> top-k without the normalise launch, identical
        # results; per-layer state = the log-normalisers the next step's scan takes its keys against.  Shapes the kernels are
        # not instantiated for (G not in {4, 8}, more than 32,768 landmarks per head) keep the three-launch path.
        self.fused_select = True
        self._sel_state = None
        self._pushed = None              # rows the host model's RoPE launch has already pushed (note_rows_pushed)
        # Reference call order (get_value_cache under copy_stream, then get_key_cache, base.py:326-338): with this flag
        # get_value_cache only returns its view and the get_key_cache call that follows for the same layer moves K AND V
        # in ONE launch on its stream (fetch_kv: rebuild tiles and landing workgroups side by side) - nothing runs on
        # copy_stream, the fork / join around it waits for nothing.  Valid for callers that do not read the V view before
        # get_key_cache has been called, which is the reference's order; off by default.
        self.lazy_value_fetch = False
        # With lazy_value_fetch: the reference-shaped methods on the IN-PLACE layout (hits keep their slots, no staging launch
        # for moved hits).  get_retrieval_position_ids then returns the slot -> chunk map in slot order instead of "hits by old
        # slot, then misses by id" - the same SET; host code that only hands the ids back to get_value_cache / get_key_cache
        # (base.py:320-338) does not see the difference.  Off by default: the default reproduces the reference's order.
        self.inplace_methods = False
        # The reference's OWN launch sequence across boundary B2: with this flag the four decode methods issue exactly the
        # calls of kv_cache.py:983-1176 - `kernels.shadowkv`'s twelve-name API (shadowkv_amd.kernels.shadowkv) and
        # tensor_op.batch_gather_gemm_rotary_pos_emb_cuda, torch.max / topk / gather between the first two - with the
        # reference's argument marshalling.  It is what a maintainer gets by swapping only the native module under the
        # reference's unmodified Python, and the form whose arguments are pinned call by call to a
        # recording of the reference itself (tests/test_decode_trace.py, tests/golden/trace_*.json).  Off by default: the
        # default methods reach the same cache bytes with fewer, fused launches.
        self.reference_calls = False
        self.gemm_o = self.softmax_o = self.norm = self.sum = None    # scratch of the reference's scoring call (:773-780)
        self._last_cos_sin = None
        self._pending_v = None           # (layer_idx, position_ids) of a deferred get_value_cache
        self._early_pub = None           # layer whose selection published an early-fetch list (consumed by fetch_kv)
        self.fetch_kv_follows = False    # set by a caller that calls fetch_kv right behind get_retrieval_position_ids
        # measurement hook (bench.py): a list -> every fetch launch of the in-place path is bracketed by two events on the
        # current stream and (start, end, layer) is appended; None (default): nothing is recorded
        self.fetch_events = None
        self.attn_out_tap = None         # test hook: see select_fetch_attend_inplace
        # Near-miss staging ahead of the next step (round 5; needs the early fetch and the fused selection): the gate/up GEMV
        # launch of every layer stages the chunks that fell just short of this step's selection (near_pull_args ->
        # tensor_op.norm_linear_decode(near_pull=)); the next step's fetch launch reads them from HBM.  Identical results.
        self.near_fetch = False
        self._near_listed = -1           # layer whose selection of this step left its near-miss lists (near_pull_args)
        self.near_pull_parts = None      # pull workgroups per (batch, head): None = about 8 in all (1 for 8 KV heads, 2 for 4)
        self.near_lists = 1              # 1: only the gate/up launch stages (ranks S+1 .. S+64); 2: the down projection stages S+65 .. S+128
        #                                  too - measured 217.3 tokens/s against 230.8 with one list (226.8 with none): the 20 us down GEMV is
        #                                  too short to hide a round of host reads (profiles/r05_near_fetch.txt)
        self._copy_stream = torch.cuda.Stream(device=self.device) if on_gpu else None

    # ------------------------------------------------------------------ bookkeeping
    def print_stats(self):
        print(f"ShadowKV_CPU | sparse budget {self.sparse_budget} | chunk size {self.chunk_size} |rank {self.rank} "
              f"| cached {self.kv_offset} | local_chunk {self.local_chunk} | outlier_chunk {self.outlier_chunk}")

    def get_kv_len(self):
        return self.kv_offset

    def clear(self):
        self.k_cache_buffer.zero_()
        self.v_cache_buffer.zero_()
        self.k_landmark = None
        self.k_landmark_scale = None
        self.k_landmark_idx = None
        self.U = None
        self.SV = None
        self.kv_offset = 0
        self.prefill = 0
        self.gen_offset = 0
        self.prefill_local = 0
        self.prefilled_batch = 0
        self.position_ids.fill_(-1)
        self._slot_age.zero_()
        self._select_ws = None          # sized for the previous landmark count
        # everything that refers to the previous prompt goes with it.  The early-fetch state is carved for that prompt's
        # landmark / chunk counts (flag tiles, early_of, staging): it is retired here (a captured step may still point at the
        # buffers: they stay allocated) and re-created for the next prompt by H2D(), so enable_early_fetch() stays a one-time
        # call for host code that clears and re-prefills per sample (test/evaluator.py:83 does)
        if self._early is not None:
            self._early_request = (self._early["E_request"], self._early["margin"])
            self._early_retired = getattr(self, "_early_retired", []) + [self._early]
            self._early = None
        self._pending_v = None
        self._early_pub = None
        self._near_listed = -1
        self._pushed = None
        self._last_cos_sin = None
        self._staged_layer = -1

    def H2D(self):
        """Reference: moves U / SV / landmarks / scratch from CPU tensors to the GPU (kv_cache.py:1178-1225).
        Here they already live in HBM; this only (re)sizes the selection workspace."""
        gc.collect()
        if self.k_landmark is not None and self.device.type == "cuda":
            n = self.k_landmark.shape[-2]
            nbytes = lib().skv_select_workspace_bytes(self.block_num, self.num_key_value_groups, n)
            self._select_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            sb = int(lib().skv_select_state_bytes(self.block_num, self.num_key_value_groups))
            if self._sel_state is None or self._sel_state.shape[1] != sb:
                self._sel_state = torch.zeros(self.num_layers, sb, dtype=torch.uint8, device=self.device)
            torch.cuda.synchronize(self.device)
            req = getattr(self, "_early_request", None)
            if req is not None and self._early is None and self.prefilled_batch == self.batch_size \
                    and self.early_fetch_supported():
                self._early_request = None
                self.enable_early_fetch(early_max=req[0], margin=req[1])

    # ------------------------------------------------------------------ prefill-side state builders
    def get_svd(self, new_k_cache, layer_idx):
        """Rank-r factorisation of the pre-RoPE keys (kv_cache.py:666-737) in f32: torch.svd (the reference's call) or the
        Gram-matrix factorisation (gram_factorize; the default for keys on a GPU - see svd_mode in __init__),
        U[:, :, :r] -> bf16, SV = diag(s) V^T stored [bs, kv, D, r] (r-contiguous for the kernels)."""
        kv, D = self.num_key_value_heads, self.head_dim
        if new_k_cache.shape[1] <= 32:   # [bs, kv, seq, D] -> [bs, seq, kv*D]  (same layout test as :683)
            k = new_k_cache.transpose(1, 2).reshape(new_k_cache.shape[0], -1, kv * D)
        else:
            k = new_k_cache
        bsz, seq = k.shape[0], k.shape[1]
        if layer_idx == 0 and self.prefilled_batch == 0:
            self.U = torch.zeros(self.num_layers, self.batch_size, seq, self.rank, device=self.device, dtype=self.dtype)
            self.SV = torch.zeros(self.num_layers, self.batch_size, kv, D, self.rank, device=self.device,
                                  dtype=self.dtype)
        r = self.rank
        b0 = self.prefilled_batch
        kf = k.float()
        mode = self.svd_mode if self.svd_mode != "auto" else ("gram" if kf.is_cuda else "svd")
        if mode == "svd":
            u, s, v = torch.svd(kf)
            self.U[layer_idx][b0:b0 + bsz].copy_(u[:, :, :r].to(self.dtype))
            sv = torch.matmul(torch.diag_embed(s[:, :r]), v.transpose(1, 2)[:, :r]).to(self.dtype)  # [bs, r, kv*D]
            del u, s, v
        else:
            u_r, sv = gram_factorize(kf, r)
            self.U[layer_idx][b0:b0 + bsz].copy_(u_r.to(self.dtype))
            sv = sv.to(self.dtype)
        self.SV[layer_idx][b0:b0 + bsz].copy_(sv.view(bsz, r, kv, D).permute(0, 2, 3, 1))

    def register_k_landmark(self, k_landmark, k_landmark_idx, layer_idx):
        n = k_landmark.shape[-2]
        bsz = k_landmark.shape[0]
        fp8 = self.landmark_dtype == "fp8_e4m3"
        if fp8 and self.head_dim != 128:
            raise ValueError("landmark_dtype='fp8_e4m3' is built for head_dim 128")
        if layer_idx == 0 and self.prefilled_batch == 0:
            shape = (self.num_layers, self.batch_size, self.num_key_value_heads, n, self.head_dim)
            if fp8:
                self.k_landmark = torch.zeros(shape, device=self.device, dtype=torch.uint8).view(torch.float8_e4m3fn)
                self.k_landmark_scale = torch.ones(shape[:-1], device=self.device, dtype=torch.float32)
            else:
                self.k_landmark = torch.zeros(shape, device=self.device, dtype=self.dtype)
            self.k_landmark_idx = torch.zeros(self.num_layers, self.batch_size, self.num_key_value_heads, n,
                                              device=self.device, dtype=torch.long)
        b0 = self.prefilled_batch
        if fp8:
            # the bf16 means, quantised by the V table's quantiser (same bytes from the native pass and the torch mirror)
            table, scale = self.k_landmark[layer_idx][b0:b0 + bsz], self.k_landmark_scale[layer_idx][b0:b0 + bsz]
            means = k_landmark.to(self.dtype)
            if means.is_cuda:
                tensor_op.quantize_v_rows(means, table.view(bsz, -1, n * self.head_dim), scale)   # straight into the table
            else:
                lm8, sc = tensor_op.quantize_v_rows_torch(means)
                table.view(torch.uint8).copy_(lm8.view(torch.uint8))
                scale.copy_(sc)
        else:
            self.k_landmark[layer_idx][b0:b0 + bsz].copy_(k_landmark)
        self.k_landmark_idx[layer_idx][b0:b0 + bsz].copy_(k_landmark_idx)

    def landmarks_bf16(self, layer_idx, b0=0, bsz=None):
        """The landmark rows the scan scores, as bf16 [bsz, kv, N, D]: the table itself, or dequant(FP8 table) (exact)."""
        b1 = self.batch_size if bsz is None else b0 + bsz
        lm = self.k_landmark[layer_idx][b0:b1]
        if self.k_landmark_scale is None:
            return lm
        return tensor_op.dequantize_v_rows(lm, self.k_landmark_scale[layer_idx][b0:b1], self.dtype)

    def _score_landmarks_torch(self, layer_idx, b0, bsz, last_q):
        """Initial selection at prefill time, in torch ops exactly as the reference does it
        (kv_cache.py:926-945): einsum / sqrt(128) -> f32 softmax -> bf16 -> max over the group -> topk."""
        kv, G, D = self.num_key_value_heads, self.num_key_value_groups, self.head_dim
        attn = torch.einsum("bhgd,bhcd->bhgc", last_q.view(-1, kv, G, D),
                            self.landmarks_bf16(layer_idx, b0, bsz).to(last_q.device)) / math.sqrt(128)
        attn = torch.nn.functional.softmax(attn, dim=-1, dtype=torch.float32).to(self.dtype)
        attn, _ = torch.max(attn, dim=-2)
        top = torch.topk(attn, k=self.select_sets, dim=-1).indices
        return self.k_landmark_idx[layer_idx][b0:b0 + bsz].to(last_q.device).gather(dim=-1, index=top)

    def prefill_kv_cache(self, new_v_cache, layer_idx, key_states_roped, last_query_states=None):
        """Builds every decode-time input of one layer from the prompt's V and post-RoPE K
        (kv_cache.py:788-980): V chunks to pinned host memory, local rows and outlier chunks to the
        buffers, landmarks (chunk means of the non-outlier chunks), the initial selection with the last
        query and the initial fill of the sparse region with exact K / V."""
        bsz, kv, incoming, D = new_v_cache.shape
        C, S = self.chunk_size, self.select_sets
        b0 = self.prefilled_batch
        self.prefill = incoming
        n_chunks_all = incoming // C
        self.max_ctx_chunks_len = n_chunks_all * C
        if self.v_scale is not None:
            self._fill_fp8_table(new_v_cache[:, :, :self.max_ctx_chunks_len], layer_idx, b0, n_chunks_all)
        else:
            self.v_cache_cpu[layer_idx][b0:b0 + bsz, :, :n_chunks_all].copy_(
                new_v_cache[:, :, :self.max_ctx_chunks_len].reshape(bsz, kv, n_chunks_all, C * D), non_blocking=True)

        self.chunks = n_chunks_all - self.local_chunk
        self.chunks -= self.chunks % 8
        ctx = self.chunks * C
        self.prefill_local = incoming - ctx
        kbuf, vbuf = self.k_cache_buffer[layer_idx][b0:b0 + bsz], self.v_cache_buffer[layer_idx][b0:b0 + bsz]
        kbuf[:, :, :self.prefill_local].copy_(key_states_roped[:, :, -self.prefill_local:])
        vbuf[:, :, :self.prefill_local].copy_(new_v_cache[:, :, -self.prefill_local:])

        k_ctx = key_states_roped[:, :, :ctx].view(bsz, kv, self.chunks, C, D)
        v_ctx = new_v_cache[:, :, :ctx].view(bsz, kv, self.chunks, C, D)
        if key_states_roped.is_cuda and C == 8 and D == 128 and key_states_roped.dtype == torch.bfloat16 \
                and key_states_roped.is_contiguous():
            # one native pass over K (skv_chunk_stats): landmark candidates + outlier score
            means, min_cos = tensor_op.chunk_stats(key_states_roped[:, :, :ctx], C)
        else:                                                                  # host mirror (CPU tests), other shapes
            means = k_ctx.mean(dim=-2)                                         # landmark candidates
            min_cos = torch.nn.functional.cosine_similarity(means.unsqueeze(3).expand(-1, -1, -1, C, -1), k_ctx,
                                                            dim=-1).min(dim=-1).values
        outlier_idx = min_cos.topk(self.outlier_chunk, largest=False).indices
        sel = outlier_idx[..., None, None].expand(-1, -1, -1, C, D)
        n_out = self.outlier_chunk * C
        self.sparse_start = self.prefill_local + n_out
        self.sparse_end = self.sparse_start + self.resident_budget   # rows of the generated tokens start here
        self.kernel_offset = self.sparse_start * D
        self.kernel_stride = self.v_cache_buffer[layer_idx].shape[-2] * D
        kbuf[:, :, self.prefill_local:self.sparse_start].copy_(k_ctx.gather(2, sel).view(bsz, kv, n_out, D))
        vbuf[:, :, self.prefill_local:self.sparse_start].copy_(v_ctx.gather(2, sel).view(bsz, kv, n_out, D))

        keep = torch.ones(bsz, kv, self.chunks, dtype=torch.bool, device=key_states_roped.device)
        keep.scatter_(-1, outlier_idx, False)
        rest_idx = torch.arange(self.chunks, device=key_states_roped.device).expand(bsz, kv, -1) \
            .masked_select(keep).view(bsz, kv, -1)
        self.register_k_landmark(means.gather(2, rest_idx.unsqueeze(-1).expand(-1, -1, -1, D)), rest_idx, layer_idx)

        chosen = self._score_landmarks_torch(layer_idx, b0, bsz, last_query_states)
        self.position_ids[layer_idx][b0:b0 + bsz, :, :S].copy_(chosen)   # slots [S, resident_sets) start empty (-1)
        pos = self.position_ids[layer_idx][b0:b0 + bsz, :, :S]
        assert pos.max() < self.chunks, f"position_ids exceed the max_length {pos.max()}"
        assert pos.min() >= 0, f"position_ids exceed the min_length {pos.min()}"
        tok = (chosen.unsqueeze(-1) * C + torch.arange(C, device=chosen.device)).view(bsz, kv, -1)
        tok = tok.unsqueeze(-1).expand(-1, -1, -1, D)
        sel_end = self.sparse_start + self.sparse_budget
        v_sel = new_v_cache.gather(-2, tok)
        if self.v_scale is not None:     # the sparse region holds what a fetch of the same chunk would land: dequant(table row)
            v_sel = self._fp8_round_trip(v_sel)
        vbuf[:, :, self.sparse_start:sel_end].copy_(v_sel, non_blocking=True)
        kbuf[:, :, self.sparse_start:sel_end].copy_(key_states_roped.gather(-2, tok), non_blocking=True)

        if layer_idx == self.num_layers - 1:
            assert self.sparse_budget < incoming
            self.prefilled_batch += bsz
            if self.prefilled_batch == self.batch_size:
                self.kv_offset += incoming
                assert not torch.any(self.position_ids[..., :S] == -1), \
                    f"The cache for offloading is not built correctly, {self.position_ids}"

    def _fill_fp8_table(self, v, layer_idx, b0, n_chunks):
        """FP8 table rows and scales of the prompt's chunks: v bf16 [bsz, kv, n_chunks * C, D] (a strided view as it comes).  On
        the GPU one native pass (skv_quantize_v_rows; the rows go straight into the table, pinned host memory included); on a
        CPU device the torch mirror.  Same bytes either way."""
        bsz = v.shape[0]
        table = self.v_cache_cpu[layer_idx][b0:b0 + bsz, :, :n_chunks]
        scale = self.v_scale[layer_idx][b0:b0 + bsz, :, :n_chunks]
        if v.is_cuda:
            tensor_op.quantize_v_rows(v, table, scale)      # (stream-ordered in front of every launch that reads the table)
        else:
            v8, sc = tensor_op.quantize_v_rows_torch(v)
            table.view(torch.uint8).copy_(v8.view(torch.uint8).reshape(bsz, -1, n_chunks, self.chunk_size * self.head_dim))
            scale.copy_(sc.view(bsz, -1, n_chunks, self.chunk_size))

    def _fp8_round_trip(self, rows):
        """dequant(quant(rows)) of bf16 token rows [bsz, kv, n, D], by the same quantiser that fills the table."""
        if rows.is_cuda:
            bsz, kv, n, D = rows.shape
            v8 = torch.empty(bsz, kv, n * D, dtype=torch.uint8, device=rows.device)
            sc = torch.empty(bsz, kv, n, dtype=torch.float32, device=rows.device)
            tensor_op.quantize_v_rows(rows, v8, sc)
            return tensor_op.dequantize_v_rows(v8.view(torch.float8_e4m3fn).view(bsz, kv, n, D), sc)
        return tensor_op.dequantize_v_rows(*tensor_op.quantize_v_rows_torch(rows))

    def _refuse_fp8_v(self, what, why):
        if self.v_scale is not None:
            raise RuntimeError(f"{what} is not available with v_dtype='fp8_e4m3': {why}")

    def _refuse_fp8_landmarks(self, what, why):
        if self.landmark_dtype != "bf16":
            raise RuntimeError(f"{what} is not available with landmark_dtype='fp8_e4m3': {why}")

    def _land_v(self, lv, what):
        """The V landing launch of the reference layout (moved hits from the staging buffer, misses from the table)."""
        vhost, vbuf = lv.vhost, lv.vbuf
        args = (ptr(vhost), ptr(vbuf), ptr(self._temp_v), ptr(self.offsets), ptr(self.cnts), vhost.stride(1), vbuf.stride(1),
                self.sparse_start * self.head_dim, self.block_num, self.select_sets)
        if self.v_scale is not None:
            check(lib().skv_land_chunks_fp8(*args, ptr(lv.vscale), lv.vscale.stride(1), current_stream_handle()), what)
        else:
            check(lib().skv_land_chunks(*args, current_stream_handle()), what)

    # ------------------------------------------------------------------ decode (native)
    class _LayerViews:
        __slots__ = ("kbuf", "vbuf", "vhost", "vscale", "lm", "lmscale", "lm_idx", "pos", "U", "SV", "cnts", "age")

    def _layer(self, l):
        """Per-layer views of the state tensors, built once (indexing a tensor makes a new view object every time: ~2 us
        each, a dozen per layer and step on the eager paths); rebuilt when a parent tensor is replaced."""
        key = (self.k_cache_buffer, self.v_cache_buffer, self.v_cache_cpu, self.k_landmark, self.k_landmark_idx,
               self.position_ids, self.U, self.SV, self.k_landmark_scale)
        old = getattr(self, "_lv_key", None)
        if old is None or any(a is not b for a, b in zip(old, key)):        # (the parents themselves are held: no id reuse)
            self._lv = []
            for i in range(self.num_layers):
                v = ShadowKVCache_CPU._LayerViews()
                v.kbuf, v.vbuf, v.vhost = self.k_cache_buffer[i], self.v_cache_buffer[i], self.v_cache_cpu[i]
                v.lm, v.lm_idx, v.pos = self.k_landmark[i], self.k_landmark_idx[i], self.position_ids[i]
                v.U, v.SV, v.cnts, v.age = self.U[i], self.SV[i], self._cnts_layers[i], self._slot_age[i]
                v.vscale = None if self.v_scale is None else self.v_scale[i]
                v.lmscale = None if self.k_landmark_scale is None else self.k_landmark_scale[i]
                self._lv.append(v)
            self._lv_key = key
        return self._lv[l]

    def _gen_rows(self, layer_idx):
        return self.gen_offset if layer_idx == self.num_layers - 1 else self.gen_offset + self.incoming_q_len

    def get_retrieval_position_ids(self, layer_idx, query_states):
        """Selects this step's chunks and diffs them against the resident set (kv_cache.py:983-1057).
        Returns position_ids[layer_idx] (reordered in place: hits by old slot, then misses by id);
        self.offsets / self.cnts are the mover's inputs."""
        self.incoming_q_len = query_states.shape[-2]
        if self.reference_calls:
            return self._ref_get_retrieval_position_ids(layer_idx, query_states)
        self._flush_pending_v()              # (a deferred V fetch reads the offsets / cnts this call is about to rewrite)
        if self.inplace_methods:
            if not self.lazy_value_fetch or self.resident_sets != self.select_sets:
                raise RuntimeError("inplace_methods needs lazy_value_fetch (K and V move in one in-place launch) and "
                                   "resident_sets == select_sets (the views cover the whole sparse region)")
            self._select_inplace(layer_idx, query_states)
            return self.position_ids[layer_idx]
        self._reference_layout_only("get_retrieval_position_ids")
        lv = self._layer(layer_idx)
        self.cnts = lv.cnts
        if self.incoming_q_len != 1:
            raise ValueError("decode-time selection expects q_len == 1 (the reference's top-k over "
                             "view(bs, kv, G, -1) is only meaningful for q_len == 1, kv_cache.py:1023-1035)")
        lm = lv.lm
        n = lm.shape[-2]
        if self._select_ws is None:
            self.H2D()
        q = query_states if query_states.is_contiguous() else query_states.contiguous()
        # early fetch in the reference's slot order: only when its consumer (fetch_kv - reached through the deferred
        # get_value_cache + get_key_cache pair, or called next by the fused step, which says so with fetch_kv_follows)
        # follows; the plain mover ignores the staging buffer
        self._early_pub = None
        if self._select_native(layer_idx, q, inplace=False, early_ok=bool(self.lazy_value_fetch or self.fetch_kv_follows)):
            self._early_pub = layer_idx
        self._stage_hits(layer_idx)
        return lv.pos

    def kv_proj_role_supported(self):
        """Whether this layer state's selection takes the k/v projection role (tensor_op.norm_q_rope): the fused two-launch
        selection of one sequence."""
        if not self.fused_select or self._sel_state is None or self.k_landmark is None or self.batch_size != 1:
            return False
        return bool(lib().skv_select_fused_supported(self.num_key_value_groups, self.k_landmark.shape[-2], self.select_sets))

    def _select_native(self, layer_idx, q, inplace, early_ok=True, kv_proj=None):
        """The selection launches of one layer (score -> [normalise] -> top-k + diff) on the current stream: the fused two-launch
        form where the kernels take the shape (skv_select_chunks_fused), else the three-launch entries.  inplace: hits keep their
        slots (offsets = miss ids, _dst_slots); else the reference's slot order.  Returns True when an early-fetch list was
        published (its consumer must be one of the *_early fetch launches of this layer)."""
        L, st = lib(), current_stream_handle()
        lv = self._layer(layer_idx)
        lm, n = lv.lm, lv.lm.shape[-2]
        ea = self._early_state() if early_ok else None
        vhost = lv.vhost
        alpha = 1.0 / math.sqrt(128)
        G, S, R = self.num_key_value_groups, self.select_sets, self.resident_sets
        if inplace and self._dst_slots is None:
            self._dst_slots = torch.zeros_like(self.offsets)
        # FP8 landmark table: the *_fp8 entries - their bf16 namesakes with the row scales behind the table
        lm_args = (ptr(lm),) if lv.lmscale is None else (ptr(lm), ptr(lv.lmscale))
        fp8 = lv.lmscale is not None
        if self.fused_select and self._sel_state is not None and L.skv_select_fused_supported(G, n, S):
            sel_args = (ptr(q), *lm_args, ptr(lv.lm_idx), ptr(lv.pos), ptr(self.offsets),
                        ptr(self._dst_slots) if inplace else 0, ptr(self.cnts), ptr(self._select_ws), 0,
                        self.block_num, G, n, S, R if inplace else S, ptr(lv.age) if inplace else 0, alpha,
                        ptr(self._sel_state[layer_idx]), 0 if ea is None else ptr(ea["states"][layer_idx]),
                        ptr(vhost), vhost.stride(1), 0 if ea is None else ea["n_chunks"],
                        0 if ea is None else ea["E"], 0.0 if ea is None else ea["margin"])
            if fp8:
                check(L.skv_select_chunks_fused_fp8(*sel_args, None if kv_proj is None else ctypes.byref(kv_proj), st),
                      "select_chunks_fused_fp8")
            elif kv_proj is not None:    # the new token's K / V row is computed by extra workgroups of one of the two launches
                check(L.skv_select_chunks_fused_kv_proj(*sel_args, ctypes.byref(kv_proj), st), "select_chunks_fused_kv_proj")
            else:
                check(L.skv_select_chunks_fused(*sel_args, st), "select_chunks_fused")
            self._near_listed = layer_idx if ea is not None else -1      # (this launch left the layer's near-miss list)
            return ea is not None
        if kv_proj is not None:
            raise RuntimeError("the k/v projection role rides in the fused selection launches only (kv_proj_role_supported)")
        if fp8 and ea is not None:
            raise RuntimeError("early fetch with landmark_dtype='fp8_e4m3' rides in the fused selection launches only "
                               "(early_fetch_supported)")
        if inplace:
            sel_args = (ptr(q), *lm_args, ptr(lv.lm_idx), ptr(lv.pos), ptr(self.offsets), ptr(self._dst_slots), ptr(self.cnts),
                        ptr(self._select_ws), 0, 0, self.block_num, G, n, S, R, ptr(lv.age), alpha)
            if ea is not None:
                check(L.skv_select_chunks_inplace_early(*sel_args, ptr(ea["states"][layer_idx]), ptr(vhost), vhost.stride(1),
                                                        ea["n_chunks"], ea["E"], ea["margin"], st), "select_chunks_inplace_early")
            elif fp8:
                check(L.skv_select_chunks_inplace_fp8(*sel_args, st), "select_chunks_inplace_fp8")
            else:
                check(L.skv_select_chunks_inplace(*sel_args, st), "select_chunks_inplace")
            return ea is not None
        if ea is not None:
            check(L.skv_select_chunks_early(ptr(q), ptr(lm), ptr(lv.lm_idx), ptr(lv.pos), ptr(self.offsets), ptr(self.cnts),
                                            ptr(self._select_ws), 0, 0, self.block_num, G, n, S, alpha, ptr(ea["states"][layer_idx]),
                                            ptr(vhost), vhost.stride(1), ea["n_chunks"], ea["E"], ea["margin"], st),
                  "get_retrieval_position_ids (early)")
            return True
        sel_args = (ptr(q), *lm_args, ptr(lv.lm_idx), ptr(lv.pos), ptr(self.offsets), ptr(self.cnts), ptr(self._select_ws), 0, 0,
                    self.block_num, G, n, S, alpha, st)
        check((L.skv_select_chunks_fp8 if fp8 else L.skv_select_chunks)(*sel_args), "get_retrieval_position_ids")
        return False

    def _reference_layout_only(self, what):
        if self.resident_sets != self.select_sets:
            raise RuntimeError(f"{what}: the reference's slot order needs resident_sets == select_sets; a larger "
                               "resident set exists in the in-place layout only (select_fetch[_attend]_inplace)")

    def _stage_hits(self, layer_idx):
        """Phase 1 of the chunk movement for BOTH buffers of a layer, once per (layer, selection): every hit
        chunk whose slot changes is copied to the staging buffers.  Must run on the stream that produced
        offsets / cnts, before the side stream forks (the fork then orders it before both landings)."""
        lv = self._layer(layer_idx)
        kbuf, vbuf = lv.kbuf, lv.vbuf
        check(lib().skv_stage_hit_chunks(ptr(kbuf), ptr(self._temp_k), ptr(vbuf), ptr(self._temp_v),
                                         ptr(self.offsets), ptr(self.cnts), kbuf.stride(1),
                                         self.sparse_start * self.head_dim, self.block_num, self.select_sets,
                                         current_stream_handle()), "stage_hit_chunks")

    def get_value_cache(self, layer_idx, position_ids):
        """Hit chunks moved to their new slots, miss chunks fetched from pinned host memory into the sparse
        region (kv_cache.py:1059-1106).  Runs on the CURRENT stream (call it under copy_stream): lands the
        hit chunks staged by get_retrieval_position_ids and pulls the misses over PCIe with plain 16-B loads
        (49-56 GB/s measured, the DMA ceiling; tools/pcie_probe.hip)."""
        if self.reference_calls:
            return self._ref_get_value_cache(layer_idx, position_ids)
        if not self.inplace_methods:
            self._reference_layout_only("get_value_cache")
        lv = self._layer(layer_idx)
        vbuf = lv.vbuf
        self._flush_pending_v()
        if self.lazy_value_fetch:
            self._pending_v = (layer_idx, position_ids)
            return vbuf[:, :, :self.sparse_end + self._gen_rows(layer_idx)]
        self._land_v(lv, "get_value_cache")
        return vbuf[:, :, :self.sparse_end + self._gen_rows(layer_idx)]

    def get_key_cache(self, layer_idx, position_ids, rope_func, cos_sin_cache):
        """Hit chunks moved to their new slots, miss chunks rebuilt as RoPE(U[idx].SV) straight into the sparse
        region (kv_cache.py:1108-1176), one launch.  `rope_func` is unused, as in the reference."""
        if self.reference_calls:
            return self._ref_get_key_cache(layer_idx, position_ids, cos_sin_cache)
        if not self.inplace_methods:
            self._reference_layout_only("get_key_cache")
        lv = self._layer(layer_idx)
        kbuf = lv.kbuf
        self._last_cos_sin = cos_sin_cache
        if self._pending_v is not None and self._pending_v[0] == layer_idx:
            self._pending_v = None
            if self.inplace_methods:
                self._fetch_inplace(layer_idx, cos_sin_cache)            # K rebuild || V fetch in place, one launch
            else:
                self.fetch_kv(layer_idx, position_ids, cos_sin_cache)    # K rebuild || V fetch, one launch, this stream
            return kbuf[:, :, :self.sparse_end + self._gen_rows(layer_idx)]
        if self.inplace_methods:
            raise RuntimeError("inplace_methods: get_key_cache must follow get_value_cache of the same layer (base.py:326-338)")
        self._flush_pending_v()
        tensor_op.rebuild_keys(lv.U, lv.SV, cos_sin_cache, position_ids, self.cnts, kbuf,
                               self.sparse_start, self.chunk_size, hit_temp=self._temp_k, hit_offsets=self.offsets)
        return kbuf[:, :, :self.sparse_end + self._gen_rows(layer_idx)]

    # ------------------------------------------------------------------ decode, the reference's own launch sequence
    def _ref_scratch(self, n):
        """gemm_o / softmax_o [bs, kv, G, n] bf16 and norm / sum [bs * kv, G, ceil(n / 256)] f32, zero-initialised: the scratch
        the reference allocates in register_k_landmark (kv_cache.py:773-780) and moves in H2D (:1211-1214)."""
        if self.gemm_o is None or self.gemm_o.shape[-1] != n:
            bs, kv, G = self.batch_size, self.num_key_value_heads, self.num_key_value_groups
            self.gemm_o = torch.zeros(bs, kv, G, n, device=self.device, dtype=self.dtype)
            self.softmax_o = torch.zeros(bs, kv, G, n, device=self.device, dtype=self.dtype)
            self.norm = torch.zeros(bs * kv, G, (n + 255) // 256, device=self.device, dtype=torch.float32)
            self.sum = torch.zeros(bs * kv, G, (n + 255) // 256, device=self.device, dtype=torch.float32)

    def _ref_guard(self, what):
        self._refuse_fp8_landmarks(f"{what} with reference_calls=True", "the reference's twelve-name API scores a bf16 table")
        self._refuse_fp8_v(f"{what} with reference_calls=True", "the reference's twelve-name API moves bf16 rows")
        if self.resident_sets != self.select_sets or self.inplace_methods or self.lazy_value_fetch:
            raise RuntimeError(f"{what}: reference_calls reproduces the reference's launch sequence, which has neither a larger "
                               "resident set nor the in-place / deferred variants")

    def _ref_get_retrieval_position_ids(self, layer_idx, query_states):
        """kv_cache.py:983-1057, call for call."""
        self._ref_guard("get_retrieval_position_ids")
        bs, kv, G = self.batch_size, self.num_key_value_heads, self.num_key_value_groups
        lm = self.k_landmark[layer_idx]
        self._ref_scratch(lm.shape[-2])
        self.cnts = self._cnts_layers[0]          # ONE counts tensor shared by all layers, as in the reference (:629)
        shadowkv.batch_gemm_softmax(query_states.contiguous(), lm.contiguous(), self.gemm_o, self.norm, self.sum,
                                    self.softmax_o, bs * kv, G * self.incoming_q_len, lm.shape[-2], self.head_dim,
                                    1 / math.sqrt(128), 0)
        chunk_attn = self.softmax_o
        if G > 1:
            chunk_attn, _ = torch.max(self.softmax_o.view(bs, kv, G, -1), dim=-2)
        top = torch.topk(chunk_attn.view(bs, kv, -1), k=self.select_sets, dim=-1).indices
        selected_chunks = self.k_landmark_idx[layer_idx].gather(dim=-1, index=top)
        shadowkv.reorder_keys_and_compute_offsets(self.position_ids[layer_idx], selected_chunks, self.offsets, self.cnts,
                                                  bs, kv, self.select_sets)
        return self.position_ids[layer_idx]

    def _ref_get_value_cache(self, layer_idx, position_ids):
        """kv_cache.py:1059-1106.  cpu_v_length: the reference passes max_ctx_chunks_len * head_dim, which IS the per-head
        stride of its V table exactly when the table was sized for this prompt (max_length // chunk_size chunks); the stride
        itself is passed here - the same number in every configuration the reference addresses correctly."""
        self._ref_guard("get_value_cache")
        vhost = self.v_cache_cpu[layer_idx]
        shadowkv.gather_copy_with_offsets(vhost, self.v_cache_buffer[layer_idx], self.temp, self.offsets, self.cnts,
                                          self.signals, self.batch_size, self.num_key_value_heads, int(vhost.stride(1)),
                                          int(self.sparse_budget * self.head_dim), self.kernel_offset, self.kernel_stride,
                                          self.select_sets)
        return self.v_cache_buffer[layer_idx][:, :, :self.sparse_end + self._gen_rows(layer_idx)]

    def _ref_get_key_cache(self, layer_idx, position_ids, cos_sin_cache):
        """kv_cache.py:1108-1176: the d2d compaction of the hits, then the two-launch rebuild (tensor_op.py:201-238)."""
        self._ref_guard("get_key_cache")
        shadowkv.gather_copy_d2d_with_offsets(self.k_cache_buffer[layer_idx], self.offsets, self.cnts, self.batch_size,
                                              self.num_key_value_heads, int(self.sparse_budget * self.head_dim),
                                              self.kernel_offset, self.kernel_stride, self.select_sets)
        tensor_op.batch_gather_gemm_rotary_pos_emb_cuda(self.U[layer_idx], self.SV[layer_idx], cos_sin_cache, position_ids,
                                                        self.output, self.chunk_size, self.k_cache_buffer[layer_idx],
                                                        self.sparse_start, self.sparse_end, self.cnts)
        return self.k_cache_buffer[layer_idx][:, :, :self.sparse_end + self._gen_rows(layer_idx)]

    def _flush_pending_v(self):
        """A get_value_cache deferred by lazy_value_fetch that was not followed by the same layer's get_key_cache: its V
        chunks are moved now, on the current stream."""
        if self._pending_v is None:
            return
        layer_idx, _ = self._pending_v
        self._pending_v = None
        if self.inplace_methods:             # (the in-place launch moves K and V together)
            if self._last_cos_sin is None:
                raise RuntimeError("inplace_methods: a deferred get_value_cache needs a get_key_cache call to carry it out")
            self._fetch_inplace(layer_idx, self._last_cos_sin)
            return
        self._land_v(self._layer(layer_idx), "get_value_cache (deferred)")

    def fetch_kv(self, layer_idx, position_ids, cos_sin_cache):
        """get_value_cache + get_key_cache of one layer as a single launch on the current stream (K rebuild
        tiles and V landing blocks run side by side inside one grid; no copy_stream fork/join).  Same bytes in
        both caches as the two separate calls."""
        self._reference_layout_only("fetch_kv")
        kbuf, vbuf = self.k_cache_buffer[layer_idx], self.v_cache_buffer[layer_idx]
        vhost = self.v_cache_cpu[layer_idx]
        U, SV = self.U[layer_idx], self.SV[layer_idx]
        width = cos_sin_cache.shape[-1]
        args = (ptr(U), ptr(SV), ptr(cos_sin_cache), ptr(position_ids), ptr(self.cnts),
                ptr(self.offsets), ptr(kbuf), ptr(self._temp_k), ptr(vhost), ptr(vbuf),
                ptr(self._temp_v), U.shape[0], self.num_key_value_heads, U.shape[1], self.head_dim,
                self.rank, self.select_sets, self.chunk_size, cos_sin_cache.stride(0), kbuf.stride(0),
                kbuf.stride(1), kbuf.stride(2), self.sparse_start, 1 if width == 128 else 2, vhost.stride(1))
        ea = self._early_state()
        if ea is not None and getattr(self, "_early_pub", None) == layer_idx:   # this step's selection published a list
            self._early_pub = None
            check(lib().skv_fetch_kv_early(*args, ptr(ea["states"][layer_idx]), self.num_key_value_groups, ea["n_lm"],
                                           ea["n_chunks"], ea["E"], current_stream_handle()), "fetch_kv (early)")
        elif self.v_scale is not None:
            vs = self.v_scale[layer_idx]
            check(lib().skv_fetch_kv_fp8(*args, ptr(vs), vs.stride(1), current_stream_handle()), "fetch_kv (fp8 V)")
        else:
            check(lib().skv_fetch_kv(*args, current_stream_handle()), "fetch_kv")

    # ------------------------------------------------------------------ decode, in-place layout (MI355X-first)
    def select_fetch_inplace(self, layer_idx, query_states, cos_sin_cache):
        """get_retrieval_position_ids + get_value_cache + get_key_cache of one layer with an IN-PLACE resident set:
        chunks selected again keep their slot, the misses take the freed slots, so no resident row moves (the
        reference compacts the hits to the front every step: kv_cache.py:1044-1057, gather_copy_d2d_with_offsets).
        Same selected set, same rows in the sparse region - in a different slot order, which attention does not see.
        4 launches (score, normalize, top-k/diff, rebuild||fetch) instead of 5; position_ids[layer_idx] stays the
        slot -> chunk map (invariant: slot i holds chunk position_ids[i])."""
        self._select_inplace(layer_idx, query_states)
        self._fetch_inplace(layer_idx, cos_sin_cache)

    def _select_inplace(self, layer_idx, query_states):
        if query_states.shape[-2] != 1:
            raise ValueError("decode-time selection expects q_len == 1")
        self.incoming_q_len = 1
        self.cnts = self._cnts_layers[layer_idx]
        lm = self.k_landmark[layer_idx]
        if self._select_ws is None:
            self.H2D()
        if self._dst_slots is None:
            self._dst_slots = torch.zeros_like(self.offsets)
        q = query_states if query_states.is_contiguous() else query_states.contiguous()
        self._select_native(layer_idx, q, inplace=True)

    def _fetch_inplace(self, layer_idx, cos_sin_cache):
        L, st = lib(), current_stream_handle()
        kbuf, vbuf = self.k_cache_buffer[layer_idx], self.v_cache_buffer[layer_idx]
        vhost = self.v_cache_cpu[layer_idx]
        U, SV = self.U[layer_idx], self.SV[layer_idx]
        width = cos_sin_cache.shape[-1]
        ev0 = self._fetch_event()
        fetch_args = (ptr(U), ptr(SV), ptr(cos_sin_cache), ptr(self.offsets), ptr(self._dst_slots),
                      ptr(self.cnts), ptr(kbuf), ptr(vhost), ptr(vbuf), U.shape[0],
                      self.num_key_value_heads, U.shape[1], self.head_dim, self.rank, self.select_sets,
                      self.chunk_size, cos_sin_cache.stride(0), kbuf.stride(0), kbuf.stride(1),
                      kbuf.stride(2), self.sparse_start, 1 if width == 128 else 2, vhost.stride(1))
        ea = self._early_state()
        if ea is not None:
            check(L.skv_fetch_kv_inplace_early(*fetch_args, ptr(ea["states"][layer_idx]), self.num_key_value_groups, ea["n_lm"],
                                               ea["n_chunks"], ea["E"], st), "fetch_kv_inplace_early")
        elif self.v_scale is not None:
            vs = self.v_scale[layer_idx]
            check(L.skv_fetch_kv_inplace_fp8(*fetch_args, ptr(vs), vs.stride(1), st), "fetch_kv_inplace (fp8 V)")
        else:
            check(L.skv_fetch_kv_inplace(*fetch_args, st), "fetch_kv_inplace")
        self._fetch_event(ev0, layer_idx)

    def _fetch_event(self, start=None, layer_idx=None):
        if self.fetch_events is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        if start is not None:
            self.fetch_events.append((start, e, layer_idx))
        return e

    def attend_slot_args(self):
        """Keyword arguments for tensor_op.sparse_attention_decode after select_fetch_inplace: with a resident set larger
        than the selection only the selected slots of the sparse region are attended."""
        if self.resident_sets == self.select_sets:
            return {}
        return dict(slots=self._dst_slots, select_sets=self.select_sets, sparse_start=self.sparse_start,
                    resident_sets=self.resident_sets)

    OVERLAP_SPLITS = 24   # split pass over the resident rows inside the fetch launch (+ one record per miss tile)

    def _overlap_splits(self):
        """~192 split-attention workgroups next to the tile workgroups whatever the batch (24 per head at bs 1, never
        fewer than 4): more would only queue behind the PCIe-bound tiles on the 256 CUs."""
        return max(4, min(self.OVERLAP_SPLITS, -(-192 // self.block_num)))

    def can_overlap_attention(self):
        # one sequence per GPU (<= 8 (batch, head) blocks): the fused launch hides the attention behind the PCIe fetch.
        # Batches are PCIe-bound outright and keep the link busier with the plain fetch launch (separate landing
        # workgroups, two per CU) + the standalone attention: measured 296 / 451 / 596 / 739 tok/s at bs 2 / 4 / 8 / 24
        # against 292 / 427 / 562 / 687 with the fused launch
        # (an FP8 V table: the fused launch's landing waves read bf16 rows - the plain launch dequantises)
        return (self.rank == 160 and self.chunk_size == 8 and self.head_dim == 128 and self.select_sets % 8 == 0
                and self.num_key_value_groups in (4, 8) and self.OVERLAP_SPLITS + self.select_sets // 8 <= 128
                and self.block_num <= 8 and self.v_scale is None)

    def early_fetch_supported(self):
        """Shapes the early-fetch roles are built for (csrc/skv_early.h): <= 65,536 landmarks and <= 1,024 resident slots per
        head, V table in pinned host memory, bf16 (the staging buffer and the roles that fill and read it move 2 KiB rows)."""
        if not (self.v_scale is None and self.k_landmark is not None and self.k_landmark.shape[-2] <= 65536 and self.resident_sets <= 1024
                and self.v_cache_cpu is not None and self.v_cache_cpu.is_pinned()):
            return False
        if self.landmark_dtype != "bf16":    # FP8 landmarks: the list role rides in the fused top-k launch only (no *_early entries)
            return bool(self.fused_select and lib().skv_select_fused_supported(self.num_key_value_groups, self.k_landmark.shape[-2],
                                                                                self.select_sets))
        return True

    def _early_state(self):
        """The early-fetch state, or None when it is off.  The state is carved for ONE prompt's landmark count, chunk count
        and block count; the selection launches carve it with the landmark table's shape and the fetch launches with the
        recorded one, so a state that no longer matches the cache (a re-prefill without clear()) is refused before any
        launch could read another layout's indices or write past its allocation."""
        ea = self._early
        if ea is None:
            return None
        n_lm = self.k_landmark.shape[-2] if self.k_landmark is not None else -1
        if ea["n_lm"] != n_lm or ea["n_chunks"] != self.v_cache_cpu.shape[-2] or ea["blocks"] != self.block_num:
            raise RuntimeError(f"early-fetch state was built for {ea['n_lm']} landmarks / {ea['n_chunks']} chunks / {ea['blocks']} "
                               f"blocks, the cache now holds {n_lm} / {self.v_cache_cpu.shape[-2]} / {self.block_num}: call "
                               "clear() before a new prefill (it retires the state) or enable_early_fetch() again")
        return ea

    @property
    def copy_stream(self):
        """The stream the reference's host code runs get_value_cache under (base.py:326-338).  With lazy_value_fetch nothing
        is launched there: the property then hands out the CURRENT stream, so the host code's wait_stream / stream switch
        become same-queue operations instead of two cross-queue hops per layer (measured: 160 -> 163 tokens/s with the
        deferred launch alone, see bench.py value_call_order)."""
        if self.lazy_value_fetch and self._copy_stream is not None:
            return torch.cuda.current_stream(self.device)
        return self._copy_stream

    def enable_early_fetch(self, early_max=None, margin=0.0, near=None):
        """Speculative early V fetch for select_fetch_attend_inplace (csrc/skv_early.hip): the scan launch flags the
        landmark slots that would have made the PREVIOUS step's top-k, an extra workgroup of the normalise launch lists up
        to `early_max` of their non-resident chunks per head, an extra workgroup of the top-k launch pulls those from the
        pinned host table while the top-k runs, and the fetch launch reads them from HBM.  Same results bit for bit; a wrong guess costs PCIe bytes only.
        early_max None: what the link moves while the top-k launch runs at the shape - 32 chunks per head for G <= 4 and 64 for
        G = 8 at 256 selected chunks per head, 1.5x per selected chunk beside it (budget 4096: 96 / 128; budget 1024: 24 / 48) - swept on
        MI355X with the fused selection (profiles/r04_fused_selection.txt: 28 / 32 / 40 / 56 chunks 222.5 / 224.8 / 224.4 / 224.1
        tokens/s at config 1; 48 / 64 / 80 198.0 / 198.0 / 195.2 at config 3; 48 / 64 / 96 / 112 / 128 173.0 / 174.2 / 179.7 / 179.9 /
        177.7 at 244K with budget 4096 - its selection runs longer, more of the link's work fits beside it; 16 / 24 / 32 261.5 / 261.8 /
        260.3 at 60K with budget 1024); 0 / False switches it off again.
        near (round 5): True / False sets `near_fetch` - the gate/up GEMV launch of every layer then also stages the chunks that
        fell just short of the step's selection for the NEXT step (near_pull_args); None leaves the attribute as it is."""
        if near is not None:
            self.near_fetch = bool(near)
        if not early_max and early_max is not None:
            if self._early is not None:      # a captured step may still point at the state buffers: they stay allocated
                self._early_retired = getattr(self, "_early_retired", []) + [self._early]
            self._early = None
            self._early_request = None
            return
        self._refuse_fp8_v("enable_early_fetch", "the early and near staging roles move 2 KiB bf16 rows")
        if not self.early_fetch_supported():
            raise RuntimeError("early fetch needs the prefilled state with the V table in pinned host memory, at most 65,536 "
                               "landmarks and at most 1,024 resident slots per head")
        L = lib()
        if early_max:
            E = int(early_max)
        elif self.block_num > 8:          # batches: what the link moves during their top-k launch, spread over all heads
            E = max(1, 256 // self.block_num)
        else:
            base = 32 if self.num_key_value_groups <= 4 else 64
            E = base if self.select_sets == 256 else max(8, base * 3 * self.select_sets // (2 * 256))
        E = max(1, min(E, 128))
        n_lm, n_chunks = self.k_landmark.shape[-2], self.v_cache_cpu.shape[-2]
        nbytes = int(L.skv_early_state_bytes(self.block_num, self.num_key_value_groups, n_lm, n_chunks, E))
        states = torch.empty(self.num_layers, nbytes, dtype=torch.uint8, device=self.device)
        st = current_stream_handle()
        for l in range(self.num_layers):
            check(L.skv_early_state_init(ptr(states[l]), self.block_num, self.num_key_value_groups, n_lm, n_chunks, E, st),
                  "early_state_init")
            # slot -> chunk id in closed form (the landmark ids are the chunk ids in ascending order minus the outliers): the
            # list role then needs no dependent gather; any other landmark_idx is detected on the device and keeps the gather
            check(L.skv_early_state_set_landmark_map(ptr(states[l]), ptr(self.k_landmark_idx[l]), self.block_num,
                                                     self.num_key_value_groups, n_lm, n_chunks, E, st), "early_state_set_landmark_map")
        offs = (ctypes.c_longlong * 13)()
        check(L.skv_early_state_offsets2(self.block_num, self.num_key_value_groups, n_lm, n_chunks, E, offs, 13), "early_state_offsets")
        torch.cuda.synchronize(self.device)
        if self._early is not None:
            self._early_retired = getattr(self, "_early_retired", []) + [self._early]
        self._early = dict(states=states, E=E, E_request=early_max, margin=float(margin), n_lm=n_lm, n_chunks=n_chunks,
                           blocks=self.block_num, offsets=list(offs))
        self._early_request = None

    def fused_select_stats(self, layer_idx):
        """Per (batch, head) of this layer's last fused selection launch: int32 [blocks, 2] = (path, candidates); path 0: the
        carried witness level held (no search, only the candidates evaluated), bit 0: the level was searched, bit 1: every
        slot was evaluated.  None when the fused selection is not in use; diagnostic, synchronises."""
        G, n = self.num_key_value_groups, self.k_landmark.shape[-2]
        if not self.fused_select or self._sel_state is None or not lib().skv_select_fused_supported(G, n, self.select_sets):
            return None
        off = int(lib().skv_select_state_stats_offset(self.block_num, G))
        return self._sel_state[layer_idx][off:off + 8 * self.block_num].view(torch.int32).view(self.block_num, 2).cpu()

    def near_pull_args(self, layer_idx, which=0):
        """Arguments of tensor_op.norm_linear_decode(..., near_pull=) for this layer's gate/up launch (which = 0: the list of
        the 64 candidates just below the selection) or of tensor_op.linear_decode(..., near_pull=) for its down projection
        (which = 1: the next 64; `near_lists` >= 2), or None when the near-miss staging is off (`near_fetch`,
        enable_early_fetch(near=True)): (early state, blocks, groups, landmarks, chunks, early_max, V table, its per-head
        stride, pull workgroups per head[, list])."""
        if which >= self.near_lists:
            return None
        ea = self._early
        if ea is None or not self.near_fetch or not self.fused_select or self._sel_state is None:
            return None
        if getattr(self, "_near_listed", -1) != layer_idx:       # this step's selection of the layer ran without the early state
            return None
        vhost = self.v_cache_cpu[layer_idx]
        args = (ptr(ea["states"][layer_idx]), ea["blocks"], self.num_key_value_groups, ea["n_lm"], ea["n_chunks"], ea["E"],
                ptr(vhost), vhost.stride(1), self.near_pull_parts or max(1, min(4, 8 // ea["blocks"])))
        return args + ((self.near_lists,) if which == 0 else (which,))      # (gate/up: how many lists are staged; down: which list)

    def near_published_ids(self, layer_idx):
        """int32 [blocks, 128]: the chunks staged AHEAD (near misses of an earlier step) in staging slots E .. E + 127
        (SKV_NEAR_SLOTS: list 0 in the first 64, list 1 in the second 64); -1 = empty."""
        e = self._early
        o, B = e["offsets"], self.block_num
        lists = e["states"][layer_idx][o[12]:o[12] + 4 * 2 * B * 64].view(torch.int32).view(2, B, 64).cpu()
        return torch.cat((lists[0], lists[1]), dim=1)

    def _early_published_ids(self, layer_idx):
        """int32 [blocks, E]: the chunk id every staging slot was PUBLISHED with in the last step of this layer, -1 = unused.
        This is the ground truth of what the fetch launch may read from staging: each pull workgroup publishes exactly the
        slots it fills (csrc/skv_early.h), whereas the state's count word comes from ONE of a head's pull workgroups, whose
        list may differ from its siblings' by a chunk when it read the resident map microseconds later."""
        e = self._early
        o, E, B = e["offsets"], e["E"], self.block_num
        return e["states"][layer_idx][o[5]:o[5] + 4 * B * E].view(torch.int32).view(B, E).cpu()

    def early_fetch_counts(self, layer_idx):
        """Chunks pulled early per (batch, head) in the last step of this layer (int32 [blocks]) = the staging slots published
        with a chunk id; diagnostic, synchronises."""
        if self._early is None:
            return None
        return (self._early_published_ids(layer_idx) >= 0).sum(dim=1).to(torch.int32)

    def early_fetch_stats(self, layer_idx):
        """(chunks pulled early, of these selected - i.e. read from staging by the fetch launch -, misses) summed over the
        heads; diagnostic, synchronises.  Valid for the layer launched LAST only (pass num_layers - 1 after a decode step):
        the miss list (self.offsets) is shared by all layers and rewritten by every layer's selection; the early ids are per
        layer (early_fetch_counts works for any layer)."""
        if self._early is None:
            return None
        B, S = self.block_num, self.select_sets
        ids = self._early_published_ids(layer_idx)
        cnts = self._cnts_layers[layer_idx].view(-1).cpu()
        miss = self.offsets.view(B, S).cpu()
        pulled = used = misses = 0
        for b in range(B):
            early = set(ids[b][ids[b] >= 0].tolist())
            m = set(miss[b, int(cnts[b]):].tolist())
            pulled += len(early); used += len(early & m); misses += len(m)
        return pulled, used, misses

    def select_fetch_attend_inplace(self, layer_idx, query_states, cos_sin_cache, kv_len=0, kv_len_dev=None, kv_proj=None):
        """select_fetch_inplace + sparse attention of one layer with the attention over the already-resident rows
        (local, outliers, surviving chunks, generated tokens) running INSIDE the fetch launch, on the CUs the PCIe-bound
        V fetch leaves idle; every miss tile (8 chunks) is attended by the workgroup that rebuilds its K rows and lands
        its V rows, straight from LDS / the landing registers; a small second launch merges the records.
        4 launches + 1 (score, normalize, top-k/diff, rebuild||fetch||attention, merge).  Returns [bs, 1, Hq, D]
        like tensor_op.sparse_attention_decode; same values up to the order of the f32 sums.
        kv_proj (tensor_op.norm_q_rope): the new token's K / V row is still to be computed - a role of the selection
        launches does it before the fetch launch attends the generated rows."""
        self._refuse_fp8_v("select_fetch_attend_inplace", "the fused launch's landing waves read bf16 rows "
                                                          "(can_overlap_attention() is False: use select_fetch_inplace)")
        if query_states.shape[-2] != 1:
            raise ValueError("decode-time selection expects q_len == 1")
        buf_rows = self.k_cache_buffer.shape[-2]
        if kv_len_dev is None and not self.sparse_end < int(kv_len) <= buf_rows:
            raise ValueError(f"kv_len {kv_len} outside ({self.sparse_end}, {buf_rows}]: the generated-row slack is "
                             f"{buf_rows - self.sparse_end} rows")
        self.incoming_q_len = 1
        self.cnts = self._cnts_layers[layer_idx]
        lm = self.k_landmark[layer_idx]
        if self._select_ws is None:
            self.H2D()
        if self._dst_slots is None:
            self._dst_slots = torch.zeros_like(self.offsets)
        q = query_states if query_states.is_contiguous() else query_states.contiguous()
        L, st = lib(), current_stream_handle()
        bs, Hq, D = q.shape[0], self.num_attention_heads, self.head_dim
        SA = self._overlap_splits()
        ws = tensor_op.attention_workspace(q.device, bs, Hq, SA + self.select_sets // 8)
        kbuf, vbuf = self.k_cache_buffer[layer_idx], self.v_cache_buffer[layer_idx]
        vhost = self.v_cache_cpu[layer_idx]
        self._select_native(layer_idx, q, inplace=True, kv_proj=kv_proj)
        ea = self._early_state()
        U, SV = self.U[layer_idx], self.SV[layer_idx]
        width = cos_sin_cache.shape[-1]
        scale = 1.0 / math.sqrt(D)
        ev0 = self._fetch_event()
        fetch_args = (ptr(U), ptr(SV), ptr(cos_sin_cache), ptr(self.offsets), ptr(self._dst_slots),
                      ptr(self.cnts), ptr(kbuf), ptr(vhost), ptr(vbuf), ptr(q), ptr(ws),
                      ptr(kv_len_dev), int(kv_len), buf_rows, U.shape[0], self.num_key_value_heads, Hq,
                      U.shape[1], D, self.rank, self.select_sets, self.chunk_size,
                      cos_sin_cache.stride(0), kbuf.stride(0), kbuf.stride(1), kbuf.stride(2),
                      self.sparse_start, 1 if width == 128 else 2, vhost.stride(1), SA,
                      self.resident_sets, scale)
        if ea is not None:
            check(L.skv_fetch_kv_attn_inplace_early(*fetch_args, ptr(ea["states"][layer_idx]), ea["n_lm"], ea["n_chunks"],
                                                    ea["E"], st), "fetch_kv_attn_inplace_early")
        else:
            check(L.skv_fetch_kv_attn_inplace(*fetch_args, st), "fetch_kv_attn_inplace")
        self._fetch_event(ev0, layer_idx)
        # (attn_out_tap: a list of per-layer [bs, 1, Hq, D] tensors a test hands in to keep every layer's attention output of
        # a captured step - the merge launch then writes there instead of into a fresh tensor; no extra launch)
        tap = self.attn_out_tap
        out = torch.empty(bs, 1, Hq, D, dtype=q.dtype, device=q.device) if tap is None else tap[layer_idx]
        check(L.skv_attn_finish_inplace(ptr(ws), ptr(self.cnts), ptr(out), bs, Hq, self.num_key_value_heads,
                                        self.select_sets, SA, st), "attn_finish_inplace")
        return out

    def note_kv_appended(self, incoming=1):
        """Bookkeeping half of update_kv_cache for callers that wrote the new K / V rows themselves
        (tensor_op.qkv_rope_update pushes them from the fused QKV kernel): advances the offsets once per token."""
        slack = self.k_cache_buffer.shape[-2] - self.sparse_end
        if self.gen_offset + incoming > slack:
            raise RuntimeError(f"generated-row slack exhausted: {self.gen_offset} + {incoming} > {slack} rows after the "
                               "sparse region (the reference silently drops such tokens, kv_cache.py:1255-1265)")
        self.kv_offset += incoming
        self.gen_offset += incoming

    def generated_row_slack(self):
        """Rows left for generated tokens behind the sparse region (buf_len - sparse_end; 96 at the 122K config)."""
        return self.k_cache_buffer.shape[-2] - self.sparse_end - self.gen_offset

    def generated_row_slack_after_prefill(self, incoming):
        """generated_row_slack() as it will be right after prefill_kv_cache of an `incoming`-token prompt (the same row
        arithmetic), so that a caller can refuse a generation length before any layer runs."""
        chunks = incoming // self.chunk_size - self.local_chunk
        chunks -= chunks % 8
        sparse_end = incoming - chunks * self.chunk_size + self.outlier_chunk * self.chunk_size + self.resident_budget
        return self.k_cache_buffer.shape[-2] - sparse_end

    def incoming_rows_writable(self, incoming):
        """True when `incoming` new rows fit behind the sparse region (a caller that pushes them itself must not write past
        the buffer; the reference drops such rows)."""
        return self.sparse_end + self.gen_offset + incoming <= self.k_cache_buffer.shape[-2]

    def note_rows_pushed(self, layer_idx, row, incoming, v_src_ptr=None):
        """The host model's RoPE launch has already written the new token's rotated K and its V into rows [row, row +
        incoming) of this layer's buffers (DecoderLM.apply_rotary_pos_emb); the update_kv_cache call that follows for the
        same layer and rows does the bookkeeping only - provided it is handed the pushed K view AND the V tensor the push
        read (v_src_ptr = its data pointer; None: any V is taken to be the pushed one)."""
        self._pushed = (layer_idx, row, incoming, v_src_ptr)

    def update_kv_cache(self, new_k_cache, new_v_cache, layer_idx):
        """Appends the new token's K / V after the sparse region (kv_cache.py:1227-1271); rows past
        the end of the buffer are dropped exactly as the reference's zero-length slice does."""
        incoming = new_k_cache.shape[-2]
        lo = self.sparse_end + self.gen_offset
        lv = self._layer(layer_idx)
        k, v = new_k_cache, new_v_cache
        pushed, self._pushed = self._pushed, None
        if (pushed is not None and pushed[:3] == (layer_idx, lo, incoming)
                and k.data_ptr() == lv.kbuf.data_ptr() + lo * self.head_dim * 2
                and (pushed[3] is None or pushed[3] == v.data_ptr())):
            pass                                                # rows already in place (see note_rows_pushed)
        elif (k.is_cuda and k.dtype == torch.bfloat16 and k.shape[-1] == 128 and k.stride(-1) == 1 and v.stride(-1) == 1
                and v.is_cuda and v.dtype == torch.bfloat16 and v.shape == k.shape
                and not ((k.stride(0) | k.stride(1) | k.stride(2) | v.stride(0) | v.stride(1) | v.stride(2)) % 8)
                and not ((k.data_ptr() | v.data_ptr()) % 16)):
            kb = lv.kbuf                                        # one native launch for both buffers
            check(lib().skv_update_kv_cache(ptr(k), ptr(v), ptr(kb), ptr(lv.vbuf), k.shape[0], k.shape[1], incoming, 128,
                                            k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2),
                                            kb.stride(0), kb.stride(1), lo, kb.shape[2], current_stream_handle()),
                  "update_kv_cache")
        else:
            lv.vbuf[:, :, lo:lo + incoming].copy_(v, non_blocking=True)
            lv.kbuf[:, :, lo:lo + incoming].copy_(k, non_blocking=True)
        if layer_idx == self.num_layers - 1:
            self.kv_offset += incoming
            self.gen_offset += incoming
