"""Thin tensor-level wrappers over the C ABI (one Python function per exported kernel).

Tensors are only used for device memory + the current stream; every call goes through
libctts_hip.so.  Inputs must live on a HIP device ("cuda" in PyTorch-ROCm) - a CPU tensor
raises: there is no CPU path in the product.

`gemm` is ctts_gemm_desc spelled out (sizes, leading dimensions, layout flags, element offsets, batch counts and strides); `bgemm` is the
same launch described by three tensor views, from which `gemm_views` derives those fields - callers that hold plain strided matrices
(attention products, bmm, slices of a packed tensor) say what they compute and cannot mis-spell a stride.
"""
import collections
import ctypes as C

import torch

from . import _lib
from ._lib import GemmDesc

ACT_NONE, ACT_RELU, ACT_GELU, ACT_TANH, ACT_SWISH = 0, 1, 2, 3, 4


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, offset=0):
    """device pointer of tensor `t` advanced by `offset` elements (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.CttsError("ctts kernels need device (HIP) tensors; got a CPU tensor - no CPU fallback exists")
    return t.data_ptr() + offset * t.element_size()


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _lib.CttsError(f"{name}: expected contiguous float32 tensor, got {t.dtype} contiguous={t.is_contiguous()}")
    return t


def _dp_rank():
    import os
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank()
    return int(os.environ.get("RANK", "0"))


class DropCtx:
    """Dropout bookkeeping: device-resident 64-bit seed + per-call-site offsets.

    The seed tensor is bumped once per step *on the device* (`advance`), so a captured
    hipGraph draws fresh masks on every replay; offsets are plain host constants assigned
    in program order, identical between eager and captured runs."""

    def __init__(self, device, seed=None):
        if seed is None:
            # follows torch.manual_seed (like nn.Dropout would) and differs per data-parallel rank: ranks that were seeded identically
            # for identical initial weights must still draw different masks
            seed = (torch.initial_seed() + 0x51ED27 * _dp_rank()) & 0x3FFFFFFFFFFF
        self.seed = torch.tensor([(int(seed) * 0x9E3779B1 + 0x7F4A7C15) & 0x7FFFFFFFFFFFFFFF], dtype=torch.int64, device=device)
        self.counter = 0

    def next_offset(self):
        self.counter = (self.counter + 1) & 0x7FFFFFFF
        return self.counter

    def begin_step(self):
        self.counter = 0

    def advance(self):
        self.seed.add_(0x632BE5AB)


import os as _os

SK_ENABLED = _os.environ.get("CTTS_SK", "1") != "0"      # persistent stream-K GEMM (csrc/gemm_sk.hip) for large unbatched launches
BF16_SPLIT = 0 if _os.environ.get("CTTS_X6", "1") == "0" else 1          # default ctts_gemm_desc.bf16_split of this module's descriptors
PLW_ENABLED = _os.environ.get("CTTS_PLW", "1") != "0"        # weight gradients on the plane kernel (csrc/gemm_plw.hip)
PLANES_ENABLED = _os.environ.get("CTTS_PL", "1") != "0"                  # pre-split operand planes + the persistent plane kernel (csrc/gemm_pl.hip)
PLANES_MIN_UNITS = int(_os.environ.get("CTTS_PL_MIN_UNITS", "4096"))
PLANES_MIN_TILES = int(_os.environ.get("CTTS_PL_MIN_TILES", "64"))
_SK_WS = {}          # (device index, stream handle) -> zero-filled workspace (include/ctts.h ctts_workspace_bytes)


def gemm_workspace(device):
    """The per-stream workspace of the library (include/ctts.h: ctts_gemm_desc.sk_ws and every `ws` argument): stream-K flags and slabs,
    split-K tickets and partial tiles, tickets and partials of the ordered column reductions.  One per (device, stream), because launches
    that share it must be stream-ordered.  Zero-filled once; every kernel leaves its flag / ticket words at zero when it finishes."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    ws = _SK_WS.get(key)
    if ws is None:
        if SK_ENABLED and not torch.cuda.is_current_stream_capturing():
            check_xcd_dispatch(device)
        ws = torch.zeros(_lib.load().ctts_workspace_bytes(), dtype=torch.uint8, device=device)
        _SK_WS[key] = ws
    return ws


_XCD_OK = {}


def check_xcd_dispatch(device):
    """Once per device: workgroup b of a launch must run on XCD b % 8 (SPX, the default compute partition of an MI355X) - the schedule
    and the slab hand-off of the persistent stream-K GEMM are built on it (nothing asserted the mode).  Any other mapping
    switches that kernel OFF for the process (the tile kernels take its launches) and says so once."""
    global SK_ENABLED
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx in _XCD_OK:
        return _XCD_OK[idx]
    out = torch.full((64,), -1, dtype=torch.int32, device=device)
    _lib.check(_lib.load().ctts_xcd_probe(_p(out), 64, _stream()), "ctts_xcd_probe")
    got = out.cpu().tolist()
    ok = got == [b % 8 for b in range(64)]
    _XCD_OK[idx] = ok
    if not ok:
        import warnings
        SK_ENABLED = False
        warnings.warn(f"ctts_amd: workgroups are not dispatched round-robin over 8 XCDs on cuda:{idx} (XCC_ID of workgroups 0..15: {got[:16]}) - "
                      "not the SPX partition mode; the persistent stream-K GEMM is disabled, the tile kernels take its launches")
    return ok


workspace = gemm_workspace


def _ws(t):
    """device pointer of the current stream's workspace on t's device"""
    return gemm_workspace(t.device).data_ptr()


class WorkspaceErrorProbe:
    """Host-side watch on the stream-K hand-off error word of every workspace in use (VERDICT r03 #2 / ADVICE r03: the owner of a cut
    tile that gives up waiting writes that word and the launch's result is garbage - nobody but the tests used to read it).
    `poll()` starts an asynchronous copy of the words into pinned memory (no sync: callable every step); `check()` waits for the last
    copy and raises CttsError if any word is set (and re-zeroes that workspace, so a later launch does not trip over a stale flag)."""

    def __init__(self):
        self._pending = []          # (workspace, pinned host word, event)

    def poll(self):
        lib = _lib.load()
        self._pending = []
        for ws in list(_SK_WS.values()):
            off = lib.ctts_workspace_error_word(C.c_void_p(ws.data_ptr())) - ws.data_ptr()
            host = torch.empty(4, dtype=torch.uint8, pin_memory=True)
            with torch.cuda.device(ws.device):
                host.copy_(ws[off:off + 4], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
            self._pending.append((ws, host, ev))

    def check(self):
        bad = []
        for ws, host, ev in self._pending:
            ev.synchronize()
            word = int(host.view(torch.int32)[0])
            if word != 0:
                bad.append((ws, word))
        self._pending = []
        for ws, word in bad:
            torch.cuda.synchronize(ws.device)
            ws.zero_()
        if bad:
            raise _lib.CttsError("stream-K GEMM hand-off failed: an owner workgroup gave up waiting for workgroup "
                                 f"{bad[0][1] - 1}'s partial tile - the results of that launch are invalid (workspace re-zeroed)")

    def poll_and_check(self):
        self.poll()
        self.check()


class PartialSink:
    """Deferred ordered reductions of a backward stage (include/ctts.h ctts_partial_sums).  While a sink is installed
    (`set_partial_sink`; trainer.TrainStep does it around every backward stage), the wrappers below that accumulate a cross-workgroup sum
    into `param.grad` - split-K weight gradients (`gemm(..., defer=True)`), bias / LayerNorm column sums - only have their kernels WRITE
    the per-workgroup partials into a scratch tensor and register (partials, count, destination) here; `flush()` then finishes all of
    them with one launch per 24 tasks, each sum in index order (bit-reproducible).  Replaces one reduce launch or one ticket tail per
    layer (fs2: ~160 per step).  The destination must not be READ before flush() - TrainStep flushes at the end of every stage, before
    the stage's gradient bucket is all-reduced."""

    # Partials are consumed while they are still in the 256 MB memory-side cache: once this many bytes are pending the sink flushes by
    # itself (a flush is legal at any point of the stage - only the END-of-stage flush is mandatory).  0 = only at the end of the stage.
    # Measured (fs2, same box): 0 / 64 / 128 / 256 MB -> 23.69 / 23.79 / 23.76 / 23.68 ms: no effect on time, the threshold only bounds the scratch.
    FLUSH_BYTES = int(float(_os.environ.get("CTTS_DEFER_FLUSH_MB", "256")) * (1 << 20))

    def __init__(self):
        self.tasks = []
        self.keep = []
        self.pending = 0
        self.streams = []          # streams the pending partials were produced on (a flush must be ordered behind ALL of them)

    def add(self, src, count, stride, n, dst, alpha, src_off=0, dst_off=0):
        d0 = dst.data_ptr() + 4 * int(dst_off)
        # a launch runs its tasks side by side as plain read-modify-write: two pending sums into overlapping destinations (a parameter
        # used by two call sites of one backward stage, tied weights) must not share a launch - finish the pending ones first
        if any(d0 < t[1] + 4 * t[2] and t[1] < d0 + 4 * int(n) for t in self.tasks):
            self.flush()
        self.tasks.append((src.data_ptr() + 4 * int(src_off), d0, int(n), int(stride), int(count), float(alpha)))
        self.keep.append((src, dst))
        if src.is_cuda:
            st = torch.cuda.current_stream(src.device)
            if st not in self.streams:
                self.streams.append(st)
        self.pending += 4 * int(count) * int(n)
        if self.FLUSH_BYTES and self.pending >= self.FLUSH_BYTES:
            self.flush()

    def flush(self):
        if not self.tasks:
            return
        arr = (_lib.PsumTask * len(self.tasks))()
        for t, (src, dst, n, stride, count, alpha) in zip(arr, self.tasks):
            t.src, t.dst, t.n, t.stride, t.count, t.alpha = src, dst, n, stride, count, alpha
        self.tasks = []
        self.pending = 0
        producers, self.streams = self.streams, []
        try:
            # The partials of a stage are written by whichever stream autograd ran the producing node on (main stream, the side stream
            # of an input-only branch).  A flush - the mandatory one at the end of the stage, or one triggered inside a node by the byte
            # threshold / an overlapping destination - reads ALL pending partials: the flushing stream waits for every other producer
            # stream first (a graph edge under capture), whichever stream it happens to be.
            cur = torch.cuda.current_stream()
            for st in producers:
                if st != cur:
                    cur.wait_stream(st)
            _lib.check(_lib.load().ctts_partial_sums(arr, len(arr), _stream()), "ctts_partial_sums")
            for src, _ in self.keep:                 # partials a side stream allocated are read by THIS stream's launch: tell the allocator
                if src.is_cuda:
                    src.record_stream(cur)
        finally:
            self.keep = []


# Bumped by every update of the parameters that autograd's version counters cannot see (dp.FlatAdam writes through raw pointers):
# per-step caches made from the weights (ops._DGRAD_W, ops._PLANES) carry the epoch they were made in.
WEIGHTS_EPOCH = [0]

_SINK = None
DEFER_ENABLED = _os.environ.get("CTTS_DEFER_SUMS", "1") != "0"       # A/B switch: 0 = every reduction finishes inside its own call


def set_partial_sink(sink):
    """install (or remove: None) the PartialSink of the current backward stage; returns the previous one"""
    global _SINK
    prev, _SINK = _SINK, (sink if DEFER_ENABLED else None)
    return prev


def _sink_for(dst):
    """the active sink if `dst` (a tensor the caller wants a sum ADDED to) is dense in memory, else None"""
    if _SINK is None or dst is None or not dst.is_contiguous():
        return None
    return _SINK


def _gemm_desc(A, B, Cout, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, a_off=0, b_off=0, c_off=0, nb0=1, nb1=1,
               sA=(0, 0), sB=(0, 0), sC=(0, 0), lens=None, lim=(0, 0, 0), conv=None, conv_on_b=False, split_k=1, alpha=1.0,
               bias=None, Z=None, ldz=0, act=ACT_NONE, p_drop=0.0, seed=None, drop_offset=0, R=None, ldr=0, rowscale=None,
               row_lens=None, row_T=0, row_halo=0, tile_map=None, E=None, rowsub=None, use_sk=None, epi_bwd=False, split_overwrite=False,
               bf16_split=None, a_planes=None, b_planes=None, c_planes=None):
    d = GemmDesc()
    if c_planes is not None:
        d.C_planes = c_planes.data_ptr()
    d.bf16_split = int(BF16_SPLIT if bf16_split is None else bf16_split)
    if a_planes is not None and b_planes is not None:
        d.A_planes, d.B_planes = a_planes.data_ptr(), b_planes.data_ptr()
    d.A, d.B, d.C = _p(A, a_off), _p(B, b_off), _p(Cout, c_off)
    d.M, d.N, d.K = int(M), int(N), int(K)
    d.lda, d.ldb, d.ldc = int(lda), int(ldb), int(ldc)
    d.a_kc, d.b_kc = int(a_kc), int(b_kc)
    d.nb0, d.nb1 = int(nb0), int(nb1)
    d.sA0, d.sA1 = int(sA[0]), int(sA[1])
    d.sB0, d.sB1 = int(sB[0]), int(sB[1])
    d.sC0, d.sC1 = int(sC[0]), int(sC[1])
    d.lens = _p(lens)
    d.lim_m, d.lim_n, d.lim_k = int(lim[0]), int(lim[1]), int(lim[2])
    if conv is not None:
        d.conv_T, d.conv_pad, d.conv_cin = int(conv[0]), int(conv[1]), int(conv[2])
        d.conv_on_b = int(conv_on_b)
    d.split_k = int(split_k)
    d.alpha = float(alpha)
    d.bias = _p(bias)
    d.Z, d.ldz = _p(Z), int(ldz)
    d.act = int(act)
    d.p_drop = float(p_drop)
    d.seed = _p(seed)
    d.drop_offset = int(drop_offset)
    d.R, d.ldr = _p(R), int(ldr)
    d.rowscale = _p(rowscale)
    if row_lens is not None:
        d.row_lens, d.row_T, d.row_halo = _p(row_lens), int(row_T), int(row_halo)
        d.tile_map = _p(tile_map)
    elif lens is not None:
        d.tile_map = _p(tile_map)          # a batch tile plan (batch_tile_map)
    d.E, d.rowsub = _p(E), _p(rowsub)
    d.epi_bwd = int(bool(epi_bwd))
    d.split_overwrite = int(bool(split_overwrite))
    if int(split_k) > 1 or a_planes is not None or ((SK_ENABLED if use_sk is None else use_sk) and nb0 * nb1 == 1 and M * N * K >= (1 << 24)):
        # split-K sums its pieces in a fixed order through the workspace (required); large unbatched GEMMs may run on the persistent
        # stream-K kernel (the library decides: ctts_gemm_sk_plan)
        ws = gemm_workspace(A.device)
        d.sk_ws, d.sk_ws_bytes = ws.data_ptr(), ws.numel()
    return d


def gemm(A, B, Cout, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, defer=False, **kw):
    """C = epi(alpha * (opA @ opB + bias)); see include/ctts.h ctts_gemm_desc (keyword arguments: _gemm_desc).
    defer=True (split_k > 1, C a dense [M, N] accumulation target such as param.grad): with a PartialSink installed the split-K partial
    matrices stay in a scratch tensor and are added to C at the sink's flush instead of by a reduce launch of their own."""
    d = _gemm_desc(A, B, Cout, M, N, K, lda, ldb, ldc, a_kc, b_kc, **kw)
    lib = _lib.load()
    if defer and _SINK is not None and d.split_k > 1 and d.nb0 * d.nb1 == 1 and ldc == N and N % 4 == 0:
        cnt, stride = C.c_int32(0), C.c_int64(0)
        if lib.ctts_gemm_split_plan(C.byref(d), C.byref(cnt), C.byref(stride)) == 1:
            P = torch.empty(d.split_k * stride.value, dtype=torch.float32, device=A.device)
            d.split_out, d.split_out_floats = P.data_ptr(), P.numel()
            _lib.check(lib.ctts_gemm(C.byref(d), _stream()), "ctts_gemm")
            _SINK.add(P, cnt.value, stride.value, M * N, Cout, d.alpha, dst_off=kw.get("c_off", 0))
            return Cout
    _lib.check(lib.ctts_gemm(C.byref(d), _stream()), "ctts_gemm")
    return Cout


def _matrix_view(t, name, nb):
    """(row_major, ld, batch strides) of the float32 view `t` [..., R, Cc] under the batch sizes `nb` of the output (broadcast like torch:
    levels are matched from the right; an absent, size-1 or expanded level has stride 0).  A matrix is row-major when its columns are
    contiguous (or there is one), column-major when its rows are; the stride of a size-1 dimension means nothing, the dense value stands
    in for it."""
    if t.dtype != torch.float32 or t.dim() < 2 or t.dim() - 2 > len(nb):
        raise _lib.CttsError(f"{name}: expected a float32 matrix view with at most {len(nb)} batch dimensions, got {t.dtype} {tuple(t.shape)}")
    (R, Cc), (sr, sc), lead = t.shape[-2:], t.stride()[-2:], t.shape[:-2]
    if sc == 1 or Cc == 1:
        row_major, ld = True, (sr if R > 1 else Cc)
    elif sr == 1 or R == 1:
        row_major, ld = False, sc
    else:
        raise _lib.CttsError(f"{name}: neither rows nor columns are contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
    if any(n not in (1, want) for n, want in zip(lead, nb[len(nb) - len(lead):])):
        raise _lib.CttsError(f"{name}: batch sizes {tuple(lead)} neither equal nor broadcast to the output's {tuple(nb)}")
    strides = [0] * (len(nb) - len(lead)) + [s if n > 1 else 0 for n, s in zip(lead, t.stride())]
    return row_major, ld, tuple(strides + [0] * (2 - len(nb)))


def gemm_views(A, B, Cout, E=None, lens=None):
    """The launch `Cout = A @ B` described by views: A = op(A) [..., M, K], B = op(B) [..., K, N], Cout [..., M, N] with 0, 1 or 2 leading
    batch dimensions -> (args, kw), the positional arguments and the nb0 / nb1 / sA / sB / sC keywords of gemm (and of gemm_route and the
    gemm_takes_* queries).  Leading dimensions, transposition flags and batch strides are read off the views; a view's data_ptr()
    includes its storage offset, so no *_off is needed.  Host-only, any device; refuses what ctts_gemm_desc cannot express.  E / lens:
    checked only (the epilogue operand must be laid out exactly like Cout, lens holds one length per nb0)."""
    nb = tuple(Cout.shape[:-2])
    if len(nb) > 2:
        raise _lib.CttsError(f"C: at most two batch dimensions, got shape {tuple(Cout.shape)}")
    (a_rm, lda, sA), (b_rm, ldb, sB), (c_rm, ldc, sC) = (_matrix_view(t, n, nb) for t, n in ((A, "A"), (B, "B"), (Cout, "C")))
    (M, Kd), N = A.shape[-2:], B.shape[-1]
    if B.shape[-2] != Kd or tuple(Cout.shape[-2:]) != (M, N):
        raise _lib.CttsError(f"inner extents disagree: A {tuple(A.shape)} @ B {tuple(B.shape)} -> C {tuple(Cout.shape)}")
    if not c_rm or (N > 1 and Cout.stride(-1) != 1):
        raise _lib.CttsError(f"C: the output needs unit column stride, got strides {Cout.stride()}")
    if E is not None and (E.shape != Cout.shape or _matrix_view(E, "E", nb) != (c_rm, ldc, sC)):
        raise _lib.CttsError(f"E: must be laid out exactly like C {tuple(Cout.shape)} {Cout.stride()}, got {tuple(E.shape)} {E.stride()}")
    nb0, nb1 = nb + (1,) * (2 - len(nb))
    if lens is not None and lens.numel() != nb0:
        raise _lib.CttsError(f"lens: {lens.numel()} lengths for nb0 = {nb0} batches")
    return (A, B, Cout, M, N, Kd, lda, ldb, ldc, a_rm, not b_rm), dict(nb0=nb0, nb1=nb1, sA=sA, sB=sB, sC=sC)


def bgemm(A, B, Cout, **kw):
    """gemm with the operands given as tensor views (gemm_views): `bgemm(P.transpose(-1, -2), dO, dV)` is dV = P^T dO.  Every other
    keyword of gemm passes through untouched."""
    args, views = gemm_views(A, B, Cout, kw.get("E"), kw.get("lens"))
    return gemm(*args, **views, **kw)


GemmRoute =collections.namedtuple("GemmRoute", "kind tile_m tile_n split_k k_granule")


def gemm_route(A, B, Cout, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, **kw):
    """The kernel ctts_gemm would run these arguments on (include/ctts.h ctts_gemm_route; no launch): GemmRoute with kind = a name of
    _lib.GEMM_KINDS, the workgroup tile, split_k as it will run and the K granule of a split.  Raises on what ctts_gemm would refuse."""
    d, info = _gemm_desc(A, B, Cout, M, N, K, lda, ldb, ldc, a_kc, b_kc, **kw), _lib.GemmRouteInfo()
    _lib.check(_lib.load().ctts_gemm_route(C.byref(d), C.byref(info)), "ctts_gemm_route")
    return GemmRoute(_lib.GEMM_KINDS[info.kind], info.tile_m, info.tile_n, info.split_k, info.k_granule)


def _gemm_takes(what, args, kw):
    """the library's ctts_gemm_takes_<what> on the descriptor of gemm(*args, **kw) (no launch)"""
    return bool(getattr(_lib.load(), "ctts_gemm_takes_" + what)(C.byref(_gemm_desc(*args, **kw))))


def gemm_takes_persistent(A, B, Cout, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, **kw):
    """True when the persistent stream-K kernel is eligible for these arguments, asked on its own (gemm_route names the kernel that runs)."""
    return SK_ENABLED and _gemm_takes("persistent", (A, B, Cout, M, N, K, lda, ldb, ldc, a_kc, b_kc), kw)


def gemm_takes_bf16_split(A, B, Cout, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, **kw):
    """True when ctts_gemm would run these arguments on the fp32-on-bf16-pipe kernel (six-term operand split; no launch)."""
    return _gemm_takes("bf16_split", (A, B, Cout, M, N, K, lda, ldb, ldc, a_kc, b_kc), kw)


def gemm_bf16_split_enable(on):
    """Default arithmetic of the descriptors this module builds (ctts_gemm_desc.bf16_split; env CTTS_X6=0 starts with it off): False =
    fp32 MFMA only, True = the large launches may run on the bf16 matrix pipe with the exact six-term operand split, 2 = also launches
    below the kernels' size thresholds (tests); "amp" (= 3; 4 without the thresholds) = the plane kernels round their operands to bf16
    and use ONE MFMA term (reference train.py:59,104 `amp.autocast` - reduced precision, never the default: see amp_split).  Returns
    the previous setting (pass it back to restore).  The library itself holds no such state any more: the choice travels in every
    descriptor, so a captured graph keeps the arithmetic it was captured with and two models can differ (`bf16_split=` on a single call
    overrides the default)."""
    global BF16_SPLIT
    prev = BF16_SPLIT
    BF16_SPLIT = 3 if on == "amp" else (int(on) if on in (2, 3, 4) else int(bool(on)))
    return prev


def amp_split():
    """`bf16_split` for a launch made under torch.amp.autocast (ops._LinearConv asks torch.is_autocast_enabled): the one-term arithmetic
    with the current setting's thresholds, or None when the bf16 kernels are switched off altogether (CTTS_X6=0 / enable(False))."""
    if BF16_SPLIT < 1:
        return None
    return 4 if BF16_SPLIT in (2, 4) else 3


def gemm_takes_planes(A, B, Cout, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, **kw):
    """True when ctts_gemm would run these arguments (a_planes / b_planes given) on the persistent plane kernel (no launch)."""
    return _gemm_takes("planes", (A, B, Cout, M, N, K, lda, ldb, ldc, a_kc, b_kc), kw)


def plane_shape_ok(M, N, K, conv_cin=None):
    """Host-side pre-filter of the plane kernel's shape rules (csrc/gemm_pl.hip ctts_gemm_pl_plan) - callers use it to decide whether splitting
    an operand is worth a launch; the library's answer (gemm_takes_planes) stays authoritative."""
    if not PLANES_ENABLED or BF16_SPLIT < 1 or not SK_ENABLED:
        return False
    if K % 32 or K < 64 or N % 128 or N < 256 or M < 128:
        return False
    if conv_cin is not None and (conv_cin % 32 or K % conv_cin):
        return False
    tiles = -(-M // 128) * -(-N // 256)
    return BF16_SPLIT in (2, 4) or (tiles * (K // 32) >= PLANES_MIN_UNITS and tiles >= PLANES_MIN_TILES)


def plane_wgrad_shape_ok(Mo, No, Kred, cin=None):
    """The same pre-filter for the weight-gradient plane kernel (csrc/gemm_plw.hip ctts_gemm_plw_plan): output [Mo, No] = [cout, k * cin], reduction
    over Kred (b, t) rows."""
    if not PLANES_ENABLED or not PLW_ENABLED or BF16_SPLIT < 1 or not SK_ENABLED:
        return False
    if Mo % 128 or No % 256 or Kred < 64:
        return False
    if cin is not None and (cin % 256 or No % cin):
        return False
    tiles = (Mo // 128) * (No // 256)
    return BF16_SPLIT in (2, 4) or (tiles >= 32 and tiles * (-(-Kred // 32)) >= PLANES_MIN_UNITS)


def split_planes(mats):
    """Exact three-way bf16 split of fp32 matrices in one launch per 32 (include/ctts.h ctts_split_planes): `mats` = list of dense 2-D
    float32 tensors [rows, cols] (cols % 32 == 0) -> list of bf16 tensors [rows, cols / 32, 3, 32]: pieces hi | mid | lo of every 32-deep
    K-block of a row side by side (the layout the plane kernel's DMA reads; `planes_piece` gives a piece back as [rows, cols])."""
    if not mats:
        return []
    outs = []
    arr = (_lib.SplitTask * len(mats))()
    for t, m in zip(arr, mats):
        _f32c(m, "split_planes operand")
        rows, cols = m.shape
        if cols % 32:
            raise _lib.CttsError(f"split_planes: cols = {cols} is not a multiple of 32")
        o = torch.empty(rows, cols // 32, 3, 32, dtype=torch.bfloat16, device=m.device)
        outs.append(o)
        t.src, t.dst, t.rows, t.cols, t.ld = _p(m), o.data_ptr(), int(rows), int(cols), int(cols)
    _lib.check(_lib.load().ctts_split_planes(arr, len(arr), _stream()), "ctts_split_planes")
    return outs


# ---- plane sets written by PRODUCERS (round 6) ------------------------------------------------------------------------------------------
# A kernel that holds an activation in registers (LayerNorm forward, BatchNorm apply / backward, the producer-epilogue backward of the
# K = 256 GEMM) can write the activation's bf16 plane set in the same launch; the set travels WITH the fp32 tensor as a Python attribute
# (autograd keeps the Python object of a tensor alive across Function boundaries, forward and backward), validated against the tensor's
# address, size and version when a GEMM asks for it.  CTTS_PRODUCER_PLANES=0: every consumer splits its own operand again (A/B switch).
PRODUCER_PLANES = _os.environ.get("CTTS_PRODUCER_PLANES", "1") != "0"


def _al16(*ts):
    return all(t.data_ptr() % 16 == 0 for t in ts)


def new_planes(rows, cols, device):
    return torch.empty(rows, cols // 32, 3, 32, dtype=torch.bfloat16, device=device)


def attach_planes(t, pl):
    t._ctts_planes = (pl, t.data_ptr(), t._version, t.numel())
    return t


def planes_of(t):
    """the plane set a producer attached to `t`, or None (never attached / `t` was written since / another tensor)"""
    ent = getattr(t, "_ctts_planes", None)
    if ent is None:
        return None
    pl, ptr, ver, n = ent
    if ptr != t.data_ptr() or ver != t._version or n != t.numel() or pl.numel() != 3 * n:
        return None
    return pl


def planes_piece(pl, q):
    """piece q (0 hi, 1 mid, 2 lo) of a plane set as a [rows, cols] bf16 tensor"""
    return pl[:, :, q, :].reshape(pl.shape[0], -1)


def gemm_takes_weight_stationary(A, B, Cout, M, N, K, lda, ldb, ldc, a_kc=True, b_kc=True, **kw):
    """True when the weight-stationary K = 256 kernel is eligible for these arguments, asked on its own (no launch)."""
    return _gemm_takes("weight_stationary", (A, B, Cout, M, N, K, lda, ldb, ldc, a_kc, b_kc), kw)


def gemm_ws_enable(on):
    """Switch of the weight-stationary K = 256 kernel (csrc/gemm_ws.hip); returns the previous setting.  Tests / A-B timing only."""
    return bool(_lib.load().ctts_gemm_ws_enable(1 if on else 0))


def row_tile_map(row_lens, row_T, row_halo, M):
    """m-tile schedule (active 64-row tiles first) for GEMMs over padded (b,t) rows; int32 [1 + ceil(M/64)]"""
    tm = torch.empty(1 + (M + 63) // 64, dtype=torch.int32, device=row_lens.device)
    lib = _lib.load()
    _lib.check(lib.ctts_row_tile_map(_p(row_lens), int(row_T), int(row_halo), int(M), _p(tm), _stream()), "ctts_row_tile_map")
    return tm


def batch_tile_map(lens, nb1, M, N, K, lim, write_all):
    """Tile plan of the batched launches with per-batch limits `lens` [nb0], `lim`, nb1 inner batches and [M, N] outputs reduced over K,
    `write_all` = their split_overwrite (include/ctts.h ctts_batch_tile_map): pass it as gemm(..., tile_map=).  None when these
    batches do not fit a plan: launch without one."""
    lib = _lib.load()
    n = lib.ctts_batch_tile_map_ints(int(lens.numel()), int(nb1), int(M), int(N))
    if n == 0:
        return None
    tm = torch.empty(n, dtype=torch.int32, device=lens.device)
    _lib.check(lib.ctts_batch_tile_map(_p(lens), int(lens.numel()), int(nb1), int(M), int(N), int(K), int(lim[0]), int(lim[1]), int(lim[2]),
                                       int(bool(write_all)), _p(tm), n, _stream()), "ctts_batch_tile_map")
    return tm


def conv_dgrad_weights(weights):
    """Data-gradient operands [Cin, K * Cout] of many Conv1d weights (GEMM-major forward layout, viewed [Cout, K * Cin]) in one launch
    per 32 layers: `weights` = list of (wmaj [Cout, K*Cin], cout, cin, k) -> list of wd tensors (include/ctts.h ctts_conv_dgrad_weights)."""
    if not weights:
        return []
    outs = [torch.empty(cin, k * cout, dtype=torch.float32, device=w.device) for w, cout, cin, k in weights]
    arr = (_lib.RepackTask * len(weights))()
    for t, (w, cout, cin, k), o in zip(arr, weights, outs):
        t.src, t.dst, t.cout, t.cin, t.k = _p(_f32c(w, "conv weight (GEMM-major)")), _p(o), int(cout), int(cin), int(k)
    _lib.check(_lib.load().ctts_conv_dgrad_weights(arr, len(arr), _stream()), "ctts_conv_dgrad_weights")
    return outs


def conv_weight_repack(src, dst, cout, cin, k, mode):
    lib = _lib.load()
    _lib.check(lib.ctts_conv_weight_repack(_p(src), _p(dst), cout, cin, k, mode, _stream()), "ctts_conv_weight_repack")
    return dst


def lr_index(dur, Tm, pad=None, round_mode=0, want_mel2ph=True):
    """-> (mel2ph int32 [B,Tm] or None, mel_len int64 [B], cum int32 [B,Ts])"""
    B, Ts = dur.shape
    is_float = dur.dtype == torch.float32
    if not is_float and dur.dtype != torch.int64:
        raise _lib.CttsError(f"lr_index: durations must be int64 or float32, got {dur.dtype}")
    dur = dur.contiguous()
    mel2ph = torch.empty(B, Tm, dtype=torch.int32, device=dur.device) if want_mel2ph else None
    mel_len = torch.empty(B, dtype=torch.int64, device=dur.device)
    cum = torch.empty(B, Ts, dtype=torch.int32, device=dur.device)
    padp = None
    if pad is not None:
        pad = pad.to(torch.uint8).contiguous()
        padp = _p(pad)
    lib = _lib.load()
    _lib.check(lib.ctts_lr_index(_p(dur), int(is_float), int(round_mode), padp, B, Ts, int(Tm), _p(mel2ph), _p(mel_len),
                                 _p(cum), _stream()), "ctts_lr_index")
    return mel2ph, mel_len, cum


def lr_gather_fwd(x, mel2ph):
    B, Ts, Cc = x.shape
    Tm = mel2ph.shape[1]
    out = torch.empty(B, Tm, Cc, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.ctts_lr_gather_fwd(_p(_f32c(x, "x")), _p(mel2ph), _p(out), B, Ts, Tm, Cc, _stream()), "ctts_lr_gather_fwd")
    return out


def lr_gather_bwd(dy, cum, Ts):
    B, Tm, Cc = dy.shape
    dx = torch.empty(B, Ts, Cc, dtype=torch.float32, device=dy.device)
    lib = _lib.load()
    _lib.check(lib.ctts_lr_gather_bwd(_p(_f32c(dy, "dy")), _p(cum), _p(dx), B, Ts, Tm, Cc, _stream()), "ctts_lr_gather_bwd")
    return dx


def positions(src, stride=1):
    """src: int64 tokens [B,T] or float32 [B,T,C] (channel 0 is tested, stride=C)."""
    B, T = src.shape[0], src.shape[1]
    pos = torch.empty(B, T, dtype=torch.int32, device=src.device)
    is_float = src.dtype == torch.float32
    lib = _lib.load()
    _lib.check(lib.ctts_positions(_p(src), int(is_float), int(stride), B, T, _p(pos), _stream()), "ctts_positions")
    return pos


def cwt_pitch(spec, f0_mean, f0_std, std_scale, eps, mel_min, mel_max, f0_bin, uv=None, uv_chan=-1, nscale=10, width=None):
    """include/ctts.h ctts_cwt_pitch: spec [B,T,C>=nscale] -> (f0 [B,width] float (log2 domain), f0_denorm [B,width] float, ids [B,width] int64)"""
    spec = _f32c(spec, "cwt_pitch spec")
    B, T, ld = spec.shape
    width = T if width is None else int(width)
    f0 = torch.empty(B, width, dtype=torch.float32, device=spec.device)
    den = torch.empty_like(f0)
    ids = torch.empty(B, width, dtype=torch.int64, device=spec.device)
    if uv is not None:
        uv = _f32c(uv if uv.dtype == torch.float32 else uv.float(), "cwt_pitch uv")
        if tuple(uv.shape) != (B, width):
            raise _lib.CttsError(f"cwt_pitch: uv has shape {tuple(uv.shape)}, expected {(B, width)}")
    f0_mean, f0_std = _f32c(f0_mean.contiguous(), "f0_mean"), _f32c(f0_std.contiguous(), "f0_std")      # named: the copies must outlive the launch
    _lib.check(_lib.load().ctts_cwt_pitch(_p(spec), ld, int(nscale), _p(f0_mean), _p(f0_std), float(std_scale),
                                          _p(uv), int(uv_chan), float(eps), float(mel_min), float(mel_max), int(f0_bin), _p(f0), _p(den), _p(ids),
                                          B, T, width, _stream()), "ctts_cwt_pitch")
    return f0, den, ids


def layernorm_fwd(x, gamma, beta, eps, p_drop=0.0, seed=None, drop_offset=0, rowscale=None, want_planes=False):
    """want_planes: also write the bf16 plane set of y (same launch) and attach it to y (`planes_of(y)`)"""
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    pl = new_planes(rows, Cc, x.device) if (want_planes and PRODUCER_PLANES and Cc % 32 == 0 and x.is_cuda) else None
    lib = _lib.load()
    _lib.check(lib.ctts_layernorm_fwd(_p(_f32c(x, "x")), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, Cc, eps,
                                      p_drop, _p(seed), drop_offset, _p(rowscale), _p(pl), _stream()), "ctts_layernorm_fwd")
    if pl is not None:
        attach_planes(y, pl)
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, p_drop=0.0, seed=None, drop_offset=0, rowscale=None, acc_into=None, dres=None):
    """acc_into=(dgamma_buf, dbeta_buf): accumulate the parameter gradients into existing buffers (param.grad)."""
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    dx = torch.empty_like(x)
    if acc_into is None:
        dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device)
    else:
        dgamma, dbeta = acc_into
    lib = _lib.load()
    sink = _sink_for(dgamma) if (acc_into is not None and dbeta.is_contiguous()) else None
    nparts = lib.ctts_reduce_parts(3, rows, Cc) if sink is not None else 0
    if nparts > 1:              # deferred: the kernel only writes its per-workgroup partial rows [dgamma | dbeta]
        parts = torch.empty(nparts, 2 * Cc, dtype=torch.float32, device=x.device)
        _lib.check(lib.ctts_layernorm_bwd(_p(_f32c(dy, "dy")), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dx), None, None, rows, Cc, p_drop,
                                          _p(seed), drop_offset, _p(rowscale), 1, _p(dres), None, _p(parts), _stream()), "ctts_layernorm_bwd")
        sink.add(parts, nparts, 2 * Cc, Cc, dgamma, 1.0)
        sink.add(parts, nparts, 2 * Cc, Cc, dbeta, 1.0, src_off=Cc)
        return dx, dgamma, dbeta
    _lib.check(lib.ctts_layernorm_bwd(_p(_f32c(dy, "dy")), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dgamma),
                                      _p(dbeta), rows, Cc, p_drop, _p(seed), drop_offset, _p(rowscale), int(acc_into is not None),
                                      _p(dres), _ws(dy), None, _stream()), "ctts_layernorm_bwd")
    return dx, dgamma, dbeta


def colstats(x2d):
    rows, Cc = x2d.shape
    sums = torch.empty(2 * Cc, dtype=torch.float64, device=x2d.device)
    lib = _lib.load()
    _lib.check(lib.ctts_colstats(_p(_f32c(x2d, "x")), _p(sums), rows, Cc, _ws(x2d), _stream()), "ctts_colstats")
    return sums


def bn_batch_stats(x2d, eps, momentum, running_mean, running_var, num_batches):
    """train-mode BatchNorm statistics of x2d [rows,C] (+ running-stat update) -> (mean, rstd) float32 [C]; two launches"""
    rows, Cc = x2d.shape
    sums = colstats(x2d)
    mean = torch.empty(Cc, dtype=torch.float32, device=x2d.device)
    rstd = torch.empty_like(mean)
    lib = _lib.load()
    _lib.check(lib.ctts_bn_finalize(_p(sums), rows, Cc, float(eps), float(momentum), _p(mean), _p(rstd), _p(running_mean),
                                    _p(running_var), _p(num_batches), _stream()), "ctts_bn_finalize")
    return mean, rstd


def bn_apply(x2d, mean, rstd, gamma, beta, act, p_drop=0.0, seed=None, drop_offset=0, want_planes=False):
    """-> y, or (y, planes of y) with want_planes (None when the shape has no plane layout)"""
    rows, Cc = x2d.shape
    y = torch.empty_like(x2d)
    pl = (new_planes(rows, Cc, x2d.device) if (want_planes and PRODUCER_PLANES and Cc % 32 == 0 and x2d.is_cuda and rows > 0
                                               and _al16(x2d, mean, rstd, gamma, beta)) else None)
    lib = _lib.load()
    _lib.check(lib.ctts_bn_apply(_p(_f32c(x2d, "x")), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(y), rows, Cc, act, p_drop,
                                 _p(seed), drop_offset, _p(pl), _stream()), "ctts_bn_apply")
    return (y, pl) if want_planes else y


def bn_bwd(dy, x2d, mean, rstd, gamma, beta, act, p_drop, seed, drop_offset, batch_stats, acc_into=None, want_planes=False):
    """acc_into = (dgamma, dbeta): existing float32 [C] buffers the parameter gradients are ADDED to (param.grad); returns (dx, None, None).
    want_planes: the bf16 plane set of dx is written by the apply launch and attached to dx (`planes_of(dx)`)."""
    rows, Cc = x2d.shape
    pl = (new_planes(rows, Cc, x2d.device) if (want_planes and PRODUCER_PLANES and Cc % 32 == 0 and x2d.is_cuda and rows > 0
                                               and _al16(dy, x2d, mean, rstd, gamma, beta)) else None)
    sums = torch.empty(2 * Cc, dtype=torch.float64, device=x2d.device)
    dx = torch.empty_like(x2d)
    if acc_into is not None:
        dgamma, dbeta = _f32c(acc_into[0], "dgamma"), _f32c(acc_into[1], "dbeta")
        batch_stats = int(batch_stats) | 2
    else:
        dgamma = torch.empty(Cc, dtype=torch.float32, device=x2d.device)
        dbeta = torch.empty(Cc, dtype=torch.float32, device=x2d.device)
    lib = _lib.load()
    _lib.check(lib.ctts_bn_bwd_reduce(_p(_f32c(dy, "dy")), _p(x2d), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(sums), rows,
                                      Cc, act, p_drop, _p(seed), drop_offset, _ws(dy), _stream()), "ctts_bn_bwd_reduce")
    _lib.check(lib.ctts_bn_bwd_apply(_p(dy), _p(x2d), _p(mean), _p(rstd), _p(gamma), _p(beta), _p(sums), _p(dx), _p(dgamma),
                                     _p(dbeta), rows, Cc, act, p_drop, _p(seed), drop_offset, int(batch_stats), _p(pl), _stream()),
               "ctts_bn_bwd_apply")
    if pl is not None:
        attach_planes(dx, pl)
    return (dx, None, None) if acc_into is not None else (dx, dgamma, dbeta)


def softmax_fwd(S, lens, nb0, nb1, T):
    lib = _lib.load()
    _lib.check(lib.ctts_softmax_fwd(_p(S), _p(lens), nb0, nb1, T, T, _stream()), "ctts_softmax_fwd")
    return S


def softmax_bwd(P, dP, lens, nb0, nb1, T):
    lib = _lib.load()
    _lib.check(lib.ctts_softmax_bwd(_p(P), _p(dP), _p(lens), nb0, nb1, T, T, _stream()), "ctts_softmax_bwd")
    return dP


def act_dropout_bwd(dg, z, act, p_drop=0.0, seed=None, drop_offset=0):
    Cc = z.shape[-1]
    rows = z.numel() // Cc
    dz = torch.empty_like(z)
    lib = _lib.load()
    _lib.check(lib.ctts_act_dropout_bwd(_p(_f32c(dg, "dg")), _p(z), _p(dz), rows, Cc, act, 1.0, p_drop, _p(seed),
                                        drop_offset, _stream()), "ctts_act_dropout_bwd")
    return dz


def rowscale_dropout(x, rowscale=None, p_drop=0.0, seed=None, drop_offset=0):
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y = torch.empty_like(x)
    lib = _lib.load()
    _lib.check(lib.ctts_rowscale_dropout(_p(_f32c(x, "x")), _p(y), rows, Cc, _p(rowscale), p_drop, _p(seed), drop_offset,
                                         _stream()), "ctts_rowscale_dropout")
    return y


def posembed_fwd(x, pos, table, alpha=None, rowscale=None, p_drop=0.0, seed=None, drop_offset=0):
    """y = rowscale * dropout(x + alpha * table[pos]); x [.., C] float32, pos int32 [rows], table [n_pos, C], alpha device scalar or None (= 1)"""
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    y = torch.empty_like(x)
    _lib.check(_lib.load().ctts_posembed_fwd(_p(_f32c(x, "x")), _p(pos), _p(_f32c(table, "table")), _p(alpha), _p(rowscale), _p(y), rows, Cc,
                                             float(p_drop), _p(seed), int(drop_offset), _stream()), "ctts_posembed_fwd")
    return y


def posembed_bwd(dy, pos, table, rowscale=None, p_drop=0.0, seed=None, drop_offset=0, want_alpha=True, alpha_acc_into=None):
    """-> (dx, dalpha [1] or None); alpha_acc_into: ADD the alpha gradient into that [1] buffer (param.grad)"""
    Cc = dy.shape[-1]
    rows = dy.numel() // Cc
    dx = torch.empty_like(dy)
    dalpha = None
    if want_alpha:
        dalpha = alpha_acc_into if alpha_acc_into is not None else torch.empty(1, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.load().ctts_posembed_bwd(_p(_f32c(dy, "dy")), _p(pos), _p(table), _p(rowscale), _p(dx), _p(dalpha), rows, Cc, float(p_drop),
                                             _p(seed), int(drop_offset), int(alpha_acc_into is not None), _ws(dy) if want_alpha else None,
                                             _stream()), "ctts_posembed_bwd")
    return dx, dalpha


def colsum(x2d, ld=None, scale=1.0, acc_into=None):
    """out[c] = scale * sum_r x[r,c]; acc_into: add into an existing buffer (param.grad) instead."""
    rows, Cc = x2d.shape
    out = torch.empty(Cc, dtype=torch.float32, device=x2d.device) if acc_into is None else acc_into
    lib = _lib.load()
    sink = _sink_for(acc_into)
    nparts = lib.ctts_reduce_parts(0, rows, Cc) if sink is not None else 0
    if nparts > 1:
        parts = torch.empty(nparts, Cc, dtype=torch.float32, device=x2d.device)
        _lib.check(lib.ctts_colsum(_p(x2d), None, rows, Cc, ld if ld is not None else Cc, 1.0, 1, None, _p(parts), _stream()), "ctts_colsum")
        sink.add(parts, nparts, Cc, Cc, out, scale)
        return out
    ldv = ld if ld is not None else Cc
    CH = 65536                                   # the kernel's column-block limit (1024 blocks of 64): wider matrices go in column chunks
    for c0 in range(0, Cc, CH):
        _lib.check(lib.ctts_colsum(_p(x2d, c0), _p(out, c0), rows, min(CH, Cc - c0), ldv, float(scale), int(acc_into is not None),
                                   _ws(x2d), None, _stream()), "ctts_colsum")
    return out


def reflect_pad(y, pad):
    """-> [B, ld] with ld = N + 2*pad rounded up to a multiple of 4 (16-B aligned rows), tail zero."""
    B, N = y.shape
    ld = (N + 2 * pad + 3) // 4 * 4
    out = torch.empty(B, ld, dtype=torch.float32, device=y.device)
    lib = _lib.load()
    _lib.check(lib.ctts_reflect_pad(_p(_f32c(y, "y")), _p(out), B, N, pad, ld, _stream()), "ctts_reflect_pad")
    return out


def stft_magnitude(reim, frames, nbins, ld_mag):
    mag = torch.empty(frames, ld_mag, dtype=torch.float32, device=reim.device)
    energy = torch.empty(frames, dtype=torch.float32, device=reim.device)
    lib = _lib.load()
    _lib.check(lib.ctts_stft_magnitude(_p(reim), reim.shape[-1], _p(mag), ld_mag, _p(energy), frames, nbins, _stream()),
               "ctts_stft_magnitude")
    return mag, energy


def log_clamp_transpose(mel_fm, B, F, n_mel, clip):
    out = torch.empty(B, n_mel, F, dtype=torch.float32, device=mel_fm.device)
    lib = _lib.load()
    _lib.check(lib.ctts_log_clamp_transpose(_p(mel_fm), _p(out), B, F, n_mel, clip, _stream()), "ctts_log_clamp_transpose")
    return out


# ------------------------------------------------------------------------- conformer kernels
def glu_fwd(a):
    C2 = a.shape[-1]
    rows = a.numel() // C2
    out = torch.empty(*a.shape[:-1], C2 // 2, dtype=torch.float32, device=a.device)
    lib = _lib.load()
    _lib.check(lib.ctts_glu_fwd(_p(_f32c(a, "a")), _p(out), rows, C2 // 2, _stream()), "ctts_glu_fwd")
    return out


def glu_bwd(a, dout):
    C2 = a.shape[-1]
    rows = a.numel() // C2
    da = torch.empty_like(a)
    lib = _lib.load()
    _lib.check(lib.ctts_glu_bwd(_p(a), _p(_f32c(dout, "dout")), _p(da), rows, C2 // 2, _stream()), "ctts_glu_bwd")
    return da


def dwconv_fwd(x, wT, flip=False):
    """x [B,T,C], wT [K,C] -> y [B,T,C] (depthwise 'same' conv; flip=True is the data gradient)."""
    B, T, Cc = x.shape
    Kk = wT.shape[0]
    y = torch.empty_like(x)
    lib = _lib.load()
    _lib.check(lib.ctts_dwconv_fwd(_p(_f32c(x, "x")), _p(_f32c(wT, "wT")), _p(y), B, T, Cc, Kk, int(flip), _stream()),
               "ctts_dwconv_fwd")
    return y


def dwconv_wgrad(dy, x, Kk, acc_into=None):
    """acc_into: existing contiguous float32 buffer of C * K elements ([C,1,K] = nn.Conv1d groups=C layout) the gradient is ADDED to"""
    B, T, Cc = x.shape
    dw = _f32c(acc_into, "dw") if acc_into is not None else torch.empty(Cc, Kk, dtype=torch.float32, device=x.device)
    partials = torch.empty(128 * Cc * 32, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.ctts_dwconv_wgrad(_p(_f32c(dy, "dy")), _p(x), _p(dw), _p(partials), B, T, Cc, Kk, int(acc_into is not None), _stream()),
               "ctts_dwconv_wgrad")
    return None if acc_into is not None else dw


def relpos_softmax_fwd(S, PS, T, scale, p_drop=0.0, seed=None, drop_offset=0, want_dropped=True):
    nb = S.numel() // (T * T)
    Pd = torch.empty_like(S) if want_dropped else None
    lib = _lib.load()
    _lib.check(lib.ctts_relpos_softmax_fwd(_p(S), _p(PS), _p(Pd), nb, T, scale, p_drop, _p(seed), drop_offset, _stream()),
               "ctts_relpos_softmax_fwd")
    return Pd


def relpos_softmax_bwd(P, dPd, T, scale, p_drop=0.0, seed=None, drop_offset=0):
    nb = P.numel() // (T * T)
    lib = _lib.load()
    _lib.check(lib.ctts_relpos_softmax_bwd(_p(P), _p(dPd), nb, T, scale, p_drop, _p(seed), drop_offset, _stream()),
               "ctts_relpos_softmax_bwd")
    return dPd


def relshift_bwd(dS, T):
    nb = dS.numel() // (T * T)
    dPS = torch.empty_like(dS)
    lib = _lib.load()
    _lib.check(lib.ctts_relshift_bwd(_p(dS), _p(dPS), nb, T, _stream()), "ctts_relshift_bwd")
    return dPS


# ------------------------------------------------------------------------- unsupervised alignment kernels
def neg_sqdist(q, k, temp):
    """q [B,Tq,C], k [B,Tk,C] -> [B,Tq,Tk] = -temp * ||q_t - k_s||^2"""
    B, Tq, Cc = q.shape
    Tk = k.shape[1]
    out = torch.empty(B, Tq, Tk, dtype=torch.float32, device=q.device)
    lib = _lib.load()
    _lib.check(lib.ctts_neg_sqdist(_p(_f32c(q, "q")), _p(_f32c(k, "k")), _p(out), B, Tq, Tk, Cc, float(temp), _stream()),
               "ctts_neg_sqdist")
    return out


def mas(attn, in_lens, out_lens):
    """attn [B,Tq,Tk] soft attention -> (hard [B,Tq,Tk] 0/1 float, dur [B,Tk] float)"""
    B, Tq, Tk = attn.shape
    opt = torch.empty_like(attn)
    dur = torch.empty(B, Tk, dtype=torch.float32, device=attn.device)
    back = torch.empty(B, Tq, Tk, dtype=torch.uint8, device=attn.device)
    lib = _lib.load()
    # keep both converted tensors alive across the launch: a temporary freed between the two conversions would hand the same
    # allocator block to the second one and the two pointers would alias
    in32 = in_lens.to(torch.int32).contiguous()
    out32 = out_lens.to(torch.int32).contiguous()
    _lib.check(lib.ctts_mas(_p(_f32c(attn, "attn")), _p(in32), _p(out32), _p(opt), _p(dur), _p(back), B, Tq, Tk, _stream()), "ctts_mas")
    return opt, dur


# ---- liu2021 prosody modelling (csrc/prosody.hip) -----------------------------------------------------------------------
def im2col_3x3s2(x):
    """x [B,T,W,C] channel-last -> col [B*T*Wo, 9*C] of Conv2d(3x3, stride (1,2), padding (1,1)); Wo = (W-1)//2+1"""
    B, T, W, Cc = x.shape
    Wo = (W - 1) // 2 + 1
    col = torch.empty(B * T * Wo, 9 * Cc, dtype=torch.float32, device=x.device)
    lib = _lib.load()
    _lib.check(lib.ctts_im2col_3x3s2(_p(_f32c(x, "x")), _p(col), B, T, W, Cc, _stream()), "ctts_im2col_3x3s2")
    return col


def col2im_3x3s2(dcol, B, T, W, Cc):
    dx = torch.empty(B, T, W, Cc, dtype=torch.float32, device=dcol.device)
    lib = _lib.load()
    _lib.check(lib.ctts_col2im_3x3s2(_p(_f32c(dcol, "dcol")), _p(dx), B, T, W, Cc, _stream()), "ctts_col2im_3x3s2")
    return dx


def gru_fwd(gi, whh, bhh, H, ndir, save_gates=True, rev_mask=None):
    """gi [B,T,ndir*3H], whh [ndir,3H,H], bhh [ndir,3H] -> (out [B,T,ndir*H], gates [B,T,ndir*4H] or None)"""
    B, T = gi.shape[0], gi.shape[1]
    out = torch.empty(B, T, ndir * H, dtype=torch.float32, device=gi.device)
    gates = torch.empty(B, T, ndir * 4 * H, dtype=torch.float32, device=gi.device) if save_gates else None
    rev_mask = (2 if ndir == 2 else 0) if rev_mask is None else int(rev_mask)       # default: nn.GRU(bidirectional) = fwd | bwd
    lib = _lib.load()
    _lib.check(lib.ctts_gru_fwd(_p(_f32c(gi, "gi")), _p(_f32c(whh, "whh")), _p(_f32c(bhh, "bhh")), _p(out), _p(gates), B, T, H, ndir,
                                rev_mask, _stream()), "ctts_gru_fwd")
    return out, gates


def gru_bwd(dout, out, gates, whh, H, ndir, rev_mask=None):
    """-> (dgi, dgh [B,T,ndir*3H], hprev [B,T,ndir*H])"""
    B, T = out.shape[0], out.shape[1]
    dgi = torch.empty(B, T, ndir * 3 * H, dtype=torch.float32, device=out.device)
    dgh = torch.empty_like(dgi)
    hprev = torch.empty_like(out)
    rev_mask = (2 if ndir == 2 else 0) if rev_mask is None else int(rev_mask)
    lib = _lib.load()
    _lib.check(lib.ctts_gru_bwd(_p(_f32c(dout, "dout")), _p(out), _p(gates), _p(_f32c(whh, "whh")), _p(dgi), _p(dgh), _p(hprev), B, T, H,
                                ndir, rev_mask, _stream()), "ctts_gru_bwd")
    return dgi, dgh, hprev


def softmax_rect_fwd(S, klens, qlens):
    """in-place masked softmax over the last dim of S [nb,Tq,Tk]; klens/qlens int32 [nb] or None"""
    nb, Tq, Tk = S.shape
    lib = _lib.load()
    _lib.check(lib.ctts_softmax_rect_fwd(_p(_f32c(S, "S")), _p(klens), _p(qlens), nb, Tq, Tk, _stream()), "ctts_softmax_rect_fwd")
    return S


def softmax_rect_bwd(P, dP, klens, qlens):
    nb, Tq, Tk = P.shape
    lib = _lib.load()
    _lib.check(lib.ctts_softmax_rect_bwd(_p(P), _p(_f32c(dP, "dP")), _p(klens), _p(qlens), nb, Tq, Tk, _stream()),
               "ctts_softmax_rect_bwd")
    return dP


def forward_sum_fwd(attn_logprob, in32, out32, blank):
    """attn_logprob [B,Tq,Tk] -> (nll [B], lse [B,Tq], alpha [B,Tq,2Tk+1])"""
    B, Tq, Tk = attn_logprob.shape
    dev = attn_logprob.device
    lse = torch.empty(B, Tq, dtype=torch.float32, device=dev)
    alpha = torch.empty(B, Tq, 2 * Tk + 1, dtype=torch.float32, device=dev)
    nll = torch.empty(B, dtype=torch.float32, device=dev)
    lib = _lib.load()
    _lib.check(lib.ctts_forward_sum_fwd(_p(_f32c(attn_logprob, "attn_logprob")), _p(in32), _p(out32), float(blank), _p(lse), _p(alpha),
                                        _p(nll), B, Tq, Tk, _stream()), "ctts_forward_sum_fwd")
    return nll, lse, alpha


def forward_sum_bwd(attn_logprob, in32, out32, blank, lse, alpha, nll, gscale):
    B, Tq, Tk = attn_logprob.shape
    grad = torch.empty_like(attn_logprob)
    lib = _lib.load()
    _lib.check(lib.ctts_forward_sum_bwd(_p(attn_logprob), _p(in32), _p(out32), float(blank), _p(lse), _p(alpha), _p(nll),
                                        _p(_f32c(gscale, "gscale")), _p(grad), B, Tq, Tk, _stream()), "ctts_forward_sum_bwd")
    return grad


def adam_clip_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, max_norm, state):
    """fused clip_grad_norm_ + Adam on flat fp32 arenas (csrc/optim.hip); lr / state are device tensors (graph-replayable)"""
    if state.numel() < _lib.ADAM_STATE_FLOATS or state.dtype != torch.float32:
        raise _lib.CttsError(f"adam_clip_step: state must hold CTTS_ADAM_STATE_FLOATS = {_lib.ADAM_STATE_FLOATS} float32 "
                             f"(got {state.numel()} {state.dtype}): the kernel writes its per-block norm partials behind the 3 scalars")
    if not (p.numel() == g.numel() == m.numel() == v.numel()):
        raise _lib.CttsError("adam_clip_step: p, g, m, v must have the same number of elements")
    lib = _lib.load()
    _lib.check(lib.ctts_adam_clip_step(_p(_f32c(p, "p")), _p(_f32c(g, "g")), _p(_f32c(m, "m")), _p(_f32c(v, "v")), p.numel(), _p(lr),
                                       float(beta1), float(beta2), float(eps), float(weight_decay), float(max_norm), _p(state),
                                       _stream()), "ctts_adam_clip_step")


def embedding_fwd(ids, weight):
    """ids int64 [...], weight [V,C] -> [..., C]"""
    V, Cc = weight.shape
    ids = ids.contiguous()
    out = torch.empty(*ids.shape, Cc, dtype=torch.float32, device=weight.device)
    lib = _lib.load()
    _lib.check(lib.ctts_embedding_fwd(_p(ids), _p(_f32c(weight, "weight")), _p(out), ids.numel(), Cc, V, _stream()), "ctts_embedding_fwd")
    return out


def embedding_bwd(ids, dy, V, padding_idx=-1, acc_into=None):
    Cc = dy.shape[-1]
    dw = torch.empty(V, Cc, dtype=torch.float32, device=dy.device) if acc_into is None else acc_into
    lib = _lib.load()
    _lib.check(lib.ctts_embedding_bwd(_p(ids), _p(_f32c(dy, "dy")), _p(dw), ids.numel(), Cc, V, int(padding_idx),
                                      int(acc_into is not None), _ws(dy), _stream()), "ctts_embedding_bwd")
    return dw


def epilogue_bwd(dy, rowscale=None, z=None, act=0, p_drop=0.0, seed=None, drop_offset=0, want_gm=False, want_bias=False,
                 bias_scale=1.0, bias_acc_into=None):
    """one-pass backward of the GEMM epilogue -> (dZ, gm or None, dbias or None); see include/ctts.h ctts_epilogue_bwd"""
    Cc = dy.shape[-1]
    rows = dy.numel() // Cc
    dz = torch.empty_like(dy)
    gm = torch.empty_like(dy) if want_gm else None
    dbias = None
    if want_bias:
        dbias = bias_acc_into if bias_acc_into is not None else torch.empty(Cc, dtype=torch.float32, device=dy.device)
    lib = _lib.load()
    sink = _sink_for(bias_acc_into) if want_bias else None
    nparts = lib.ctts_reduce_parts(2, rows, Cc) if sink is not None else 0
    if nparts > 1:              # deferred bias gradient: per-stripe partial rows, added at the sink's flush
        parts = torch.empty(nparts, Cc, dtype=torch.float32, device=dy.device)
        _lib.check(lib.ctts_epilogue_bwd(_p(_f32c(dy, "dy")), _p(rowscale), _p(z if act else None), _p(dz), _p(gm), None, rows, Cc,
                                         int(act), float(p_drop), _p(seed), int(drop_offset), 1.0, 1, None, _p(parts), _stream()),
                   "ctts_epilogue_bwd")
        sink.add(parts, nparts, Cc, Cc, dbias, bias_scale)
        return dz, gm, dbias
    _lib.check(lib.ctts_epilogue_bwd(_p(_f32c(dy, "dy")), _p(rowscale), _p(z if act else None), _p(dz), _p(gm), _p(dbias), rows, Cc,
                                     int(act), float(p_drop), _p(seed), int(drop_offset), float(bias_scale),
                                     int(bias_acc_into is not None), _ws(dy) if want_bias else None, None, _stream()), "ctts_epilogue_bwd")
    return dz, gm, dbias


def rowdot_heads(a, b, n_heads):
    """a, b [B,T,C] -> [B,H,T]: per-head dot products along the channel slices (D = rowsum(dO * O) of the fused softmax backward)"""
    B, T, Cc = a.shape
    out = torch.empty(B, n_heads, T, dtype=torch.float32, device=a.device)
    lib = _lib.load()
    _lib.check(lib.ctts_rowdot_heads(_p(_f32c(a, "a")), _p(_f32c(b, "b")), _p(out), B, T, n_heads, Cc // n_heads, _stream()),
               "ctts_rowdot_heads")
    return out


# ---- fused attention (csrc/attn.hip) -------------------------------------------------------------------------------------
def mha_supported(C, H):
    return bool(_lib.load().ctts_mha_supported(int(C), int(H)))


def mha_fwd(qkv, lens, n_heads, scale):
    """qkv [B,T,3C] packed projections, lens int32 [B] or None -> (out [B,T,C], lse [B,H,T])"""
    B, T, C3 = qkv.shape
    Cc = C3 // 3
    out = torch.empty(B, T, Cc, dtype=torch.float32, device=qkv.device)
    lse = torch.empty(B, n_heads, T, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    _lib.check(lib.ctts_mha_fwd(_p(_f32c(qkv, "qkv")), _p(lens), _p(out), _p(lse), B, T, n_heads, Cc, float(scale), _stream()), "ctts_mha_fwd")
    return out, lse


def mha_bwd(qkv, lens, out, dout, lse, n_heads, scale, q_split=1):
    """-> dqkv [B,T,3C]"""
    B, T, C3 = qkv.shape
    Cc = C3 // 3
    dev = qkv.device
    dqkv = torch.empty_like(qkv)
    Dws = torch.empty(B, n_heads, T, dtype=torch.float32, device=dev)
    dS = torch.empty(B, n_heads, T, T, dtype=torch.float32, device=dev)
    part = torch.empty(q_split, B, T, 2 * Cc, dtype=torch.float32, device=dev) if q_split > 1 else None
    lib = _lib.load()
    _lib.check(lib.ctts_mha_bwd(_p(qkv), _p(lens), _p(_f32c(out, "out")), _p(_f32c(dout, "dout")), _p(lse), _p(Dws), _p(dS), _p(part), _p(dqkv),
                                B, T, n_heads, Cc, float(scale), int(q_split), _ws(qkv), _stream()), "ctts_mha_bwd")
    return dqkv


def relattn_split_fwd(qkv, u_bias, v_bias):
    """packed q | k | v projection [..., 3C] -> (qu = q + u_bias, qv = q + v_bias [..., C], kv [..., 2C])"""
    Cc = qkv.shape[-1] // 3
    rows = qkv.numel() // (3 * Cc)
    qu = torch.empty(*qkv.shape[:-1], Cc, dtype=torch.float32, device=qkv.device)
    qv = torch.empty_like(qu)
    kv = torch.empty(*qkv.shape[:-1], 2 * Cc, dtype=torch.float32, device=qkv.device)
    _lib.check(_lib.load().ctts_relattn_split_fwd(_p(_f32c(qkv, "qkv")), _p(_f32c(u_bias, "u_bias")), _p(_f32c(v_bias, "v_bias")), _p(qu), _p(qv),
                                                  _p(kv), rows, Cc, _stream()), "ctts_relattn_split_fwd")
    return qu, qv, kv


def relattn_split_bwd(dqu, dqv, dkv):
    """-> dqkv [..., 3C] = (dqu + dqv) | dkv"""
    Cc = dqu.shape[-1]
    rows = dqu.numel() // Cc
    dqkv = torch.empty(*dqu.shape[:-1], 3 * Cc, dtype=torch.float32, device=dqu.device)
    _lib.check(_lib.load().ctts_relattn_split_bwd(_p(_f32c(dqu, "dqu")), _p(_f32c(dqv, "dqv")), _p(_f32c(dkv, "dkv")), _p(dqkv), rows, Cc,
                                                  _stream()), "ctts_relattn_split_bwd")
    return dqkv


def relmha_fwd(qu, qv, kv, pos, n_heads, scale, p_drop=0.0, seed=None, drop_offset=0):
    """-> (out [B,T,C], lse [B,H,T])"""
    B, T, Cc = qu.shape
    dev = qu.device
    lib = _lib.load()
    out = torch.empty(B, T, Cc, dtype=torch.float32, device=dev)
    lse = torch.empty(B, n_heads, T, dtype=torch.float32, device=dev)
    _lib.check(lib.ctts_relmha_fwd(_p(_f32c(qu, "qu")), _p(_f32c(qv, "qv")), _p(_f32c(kv, "kv")), _p(_f32c(pos, "pos")), _p(out),
                                   _p(lse), B, T, n_heads, Cc, float(scale), float(p_drop), _p(seed), int(drop_offset), _stream()),
               "ctts_relmha_fwd")
    return out, lse


def relmha_bwd(qu, qv, kv, pos, out, dout, lse, n_heads, scale, p_drop=0.0, seed=None, drop_offset=0):
    """-> (dqu, dqv [B,T,C], dkv [B,T,2C], dpos_b [B,T,C])"""
    B, T, Cc = qu.shape
    dev = qu.device
    lib = _lib.load()
    Dws = torch.empty(B, n_heads, T, dtype=torch.float32, device=dev)
    dS = torch.empty(lib.ctts_relmha_workspace_floats(B, T, n_heads), dtype=torch.float32, device=dev)
    dqu, dqv, dkv = torch.empty_like(qu), torch.empty_like(qv), torch.empty_like(kv)
    dpos_b = torch.empty(B, T, Cc, dtype=torch.float32, device=dev)
    _lib.check(lib.ctts_relmha_bwd(_p(qu), _p(qv), _p(kv), _p(pos), _p(_f32c(out, "out")), _p(_f32c(dout, "dout")), _p(lse), _p(Dws),
                                   _p(dS), _p(dqu), _p(dqv), _p(dkv), _p(dpos_b), B, T, n_heads, Cc, float(scale), float(p_drop),
                                   _p(seed), int(drop_offset), _stream()), "ctts_relmha_bwd")
    return dqu, dqv, dkv, dpos_b


def weighted_colsum(x2d, w, scale=1.0, acc_into=None):
    """out[c] = scale * sum_r w[r] * x[r,c]"""
    rows, Cc = x2d.shape
    out = torch.empty(Cc, dtype=torch.float32, device=x2d.device) if acc_into is None else acc_into
    lib = _lib.load()
    sink = _sink_for(acc_into)
    nparts = lib.ctts_reduce_parts(1, rows, Cc) if sink is not None else 0
    if nparts > 1:
        parts = torch.empty(nparts, Cc, dtype=torch.float32, device=x2d.device)
        _lib.check(lib.ctts_weighted_colsum(_p(_f32c(x2d, "x")), _p(_f32c(w, "w")), None, rows, Cc, 1.0, 1, None, _p(parts), _stream()),
                   "ctts_weighted_colsum")
        sink.add(parts, nparts, Cc, Cc, out, scale)
        return out
    _lib.check(lib.ctts_weighted_colsum(_p(_f32c(x2d, "x")), _p(_f32c(w, "w")), _p(out), rows, Cc, float(scale),
                                        int(acc_into is not None), _ws(x2d), None, _stream()), "ctts_weighted_colsum")
    return out


def mel_l1_fwd(p1, p2, tgt, pad_u8):
    """-> (sums [3] = {sum w|p1-t|, sum w|p2-t|, sum w}, roww [rows])"""
    Cc = tgt.shape[-1]
    rows = tgt.numel() // Cc
    sums = torch.empty(3, dtype=torch.float32, device=tgt.device)        # written by the workgroup that finishes the ordered sum
    roww = torch.empty(rows, dtype=torch.float32, device=tgt.device)
    lib = _lib.load()
    _lib.check(lib.ctts_mel_l1_fwd(_p(_f32c(p1, "p1")), _p(_f32c(p2, "p2")), _p(_f32c(tgt, "tgt")), _p(pad_u8), _p(sums), _p(roww), rows,
                                   Cc, _ws(tgt), _stream()), "ctts_mel_l1_fwd")
    return sums, roww


def mel_l1_bwd(p1, p2, tgt, roww, sums, g):
    Cc = tgt.shape[-1]
    rows = tgt.numel() // Cc
    d1, d2 = torch.empty_like(p1), torch.empty_like(p2)
    lib = _lib.load()
    _lib.check(lib.ctts_mel_l1_bwd(_p(p1), _p(p2), _p(tgt), _p(roww), _p(sums), _p(_f32c(g, "g")), _p(d1), _p(d2), rows, Cc, _stream()),
               "ctts_mel_l1_bwd")
    return d1, d2


# ---- fused variance / duration loss terms (csrc/loss.hip) ----------------------------------------------------------------
def _var_loss_args(log_d, dur, texts, src_pad, cwt, cwt_spec, uv, mel_pad, f0m_p, f0m_t, f0s_p, f0s_t, e_pred, e_tgt):
    B, Ts = log_d.shape
    Tm = cwt.shape[1]
    if texts.dtype != torch.int64:
        raise _lib.CttsError(f"var_loss: texts must be int64 token ids, got {texts.dtype}")
    if dur.dtype not in (torch.int64, torch.float32):
        raise _lib.CttsError(f"var_loss: durations must be int64 or float32, got {dur.dtype}")
    if cwt.shape[-1] != 11 or cwt_spec.shape[-1] != 10:
        raise _lib.CttsError("var_loss: expected cwt [B,Tm,11] (10 bins + uv logit) and cwt_spec [B,Tm,10]")
    ptrs = [_p(_f32c(log_d, "log_d")), _p(dur), int(dur.dtype == torch.float32), _p(texts), _p(src_pad), _p(_f32c(cwt, "cwt")),
            _p(_f32c(cwt_spec, "cwt_spec")), _p(_f32c(uv, "uv")), _p(mel_pad), _p(_f32c(f0m_p, "f0_mean")), _p(_f32c(f0m_t, "f0_mean tgt")),
            _p(_f32c(f0s_p, "f0_std")), _p(_f32c(f0s_t, "f0_std tgt")), _p(_f32c(e_pred, "e_pred")), _p(_f32c(e_tgt, "e_tgt")), B, Ts, Tm]
    return ptrs, B, Ts, Tm


def _check_var_loss_host_args(lambdas_t, sil_t):
    """the C ABI reads lambdas5[0..4] and sil_ids3[0..2] through HOST pointers at launch"""
    if lambdas_t.is_cuda or sil_t.is_cuda:
        raise _lib.CttsError("var_loss: lambdas / silence ids must be HOST tensors (the library reads them at launch); a .to(device) on "
                             "the loss module must not move them")
    if lambdas_t.dtype != torch.float32 or lambdas_t.numel() != 5 or not lambdas_t.is_contiguous():
        raise _lib.CttsError(f"var_loss: lambdas must be 5 contiguous float32, got {lambdas_t.numel()} {lambdas_t.dtype}")
    if sil_t.dtype != torch.int64 or sil_t.numel() != 3 or not sil_t.is_contiguous():
        raise _lib.CttsError(f"var_loss: silence ids must be 3 contiguous int64 (loss.py:149), got {sil_t.numel()} {sil_t.dtype}")


def var_loss_fwd(tensors, lambdas_t, cwt_l2, sil_t):
    """tensors = (log_d, dur, texts, src_pad u8, cwt, cwt_spec, uv, mel_pad u8, f0m_p, f0m_t, f0s_p, f0s_t, e_pred, e_tgt);
    lambdas_t float32 [5] and sil_t int64 [3] are HOST tensors (read at launch).  -> (terms [8], partials, wsum, denoms)"""
    _check_var_loss_host_args(lambdas_t, sil_t)
    ptrs, B, Ts, Tm = _var_loss_args(*tensors)
    dev = tensors[0].device
    partials = torch.empty(B, 16, dtype=torch.float32, device=dev)
    wsum = torch.empty(B, 2, Ts + 1, dtype=torch.float32, device=dev)
    terms = torch.empty(8, dtype=torch.float32, device=dev)
    denoms = torch.empty(4, dtype=torch.float32, device=dev)
    lib = _lib.load()
    _lib.check(lib.ctts_var_loss_fwd(*ptrs, lambdas_t.data_ptr(), int(cwt_l2), sil_t.data_ptr(), _p(partials), _p(wsum), _p(terms),
                                     _p(denoms), _stream()), "ctts_var_loss_fwd")
    return terms, partials, wsum, denoms


def var_loss_bwd(tensors, lambdas_t, cwt_l2, sil_t, partials, wsum, denoms, g8):
    _check_var_loss_host_args(lambdas_t, sil_t)
    ptrs, B, Ts, Tm = _var_loss_args(*tensors)
    dev = tensors[0].device
    d_log_d = torch.empty(B, Ts, dtype=torch.float32, device=dev)
    d_e = torch.empty(B, Ts, dtype=torch.float32, device=dev)
    d_cwt = torch.empty(B, Tm, 11, dtype=torch.float32, device=dev)
    d_f0m = torch.empty(B, dtype=torch.float32, device=dev)
    d_f0s = torch.empty(B, dtype=torch.float32, device=dev)
    lib = _lib.load()
    _lib.check(lib.ctts_var_loss_bwd(*ptrs, lambdas_t.data_ptr(), int(cwt_l2), sil_t.data_ptr(), _p(partials), _p(wsum), _p(denoms),
                                     _p(_f32c(g8, "g8")), _p(d_log_d), _p(d_cwt), _p(d_f0m), _p(d_f0s), _p(d_e), _stream()),
               "ctts_var_loss_bwd")
    return d_log_d, d_cwt, d_f0m, d_f0s, d_e


def bin_loss_fwd(soft, hard):
    n = soft.numel()
    partials = torch.empty(1024, dtype=torch.float32, device=soft.device)
    out2 = torch.empty(2, dtype=torch.float32, device=soft.device)
    lib = _lib.load()
    _lib.check(lib.ctts_bin_loss_fwd(_p(_f32c(soft, "soft")), _p(_f32c(hard, "hard")), n, _p(partials), _p(out2), _stream()), "ctts_bin_loss_fwd")
    return out2


def bin_loss_bwd(soft, hard, out2, g):
    dsoft = torch.empty_like(soft)
    lib = _lib.load()
    _lib.check(lib.ctts_bin_loss_bwd(_p(soft), _p(hard), _p(out2), _p(_f32c(g, "g")), _p(dsoft), soft.numel(), _stream()), "ctts_bin_loss_bwd")
    return dsoft


MASKED_L1, MASKED_L2, MASKED_BCE = 0, 1, 2


def masked_loss_fwd(pred, target, weight, kind):
    n = pred.numel()
    partials = torch.empty(1024, dtype=torch.float32, device=pred.device)
    out2 = torch.empty(2, dtype=torch.float32, device=pred.device)
    lib = _lib.load()
    _lib.check(lib.ctts_masked_loss_fwd(_p(_f32c(pred, "pred")), _p(_f32c(target, "target")), _p(_f32c(weight, "weight")), n, int(kind),
                                        _p(partials), _p(out2), _stream()), "ctts_masked_loss_fwd")
    return out2


def masked_loss_bwd(pred, target, weight, out2, g, kind):
    dpred = torch.empty_like(pred)
    lib = _lib.load()
    _lib.check(lib.ctts_masked_loss_bwd(_p(pred), _p(target), _p(weight), _p(out2), _p(_f32c(g, "g")), _p(dpred), pred.numel(), int(kind),
                                        _stream()), "ctts_masked_loss_bwd")
    return dpred


# ---- mel front end as a real FFT (csrc/mel.hip) ------------------------------------------------------------------------------
def mel_prepare(mel_basis, n_fft):
    """-> workspace tensor for `mel_spectrogram_fft` (twiddles, transposed filterbank, per-tile bin ranges)"""
    n_mel = mel_basis.shape[0]
    lib = _lib.load()
    ws = torch.empty(lib.ctts_mel_spectrogram_workspace_bytes(int(n_fft), int(n_mel)) // 4, dtype=torch.float32, device=mel_basis.device)
    _lib.check(lib.ctts_mel_prepare(_p(_f32c(mel_basis, "mel_basis")), int(n_fft), int(n_mel), _p(ws), _stream()), "ctts_mel_prepare")
    return ws


def mel_spectrogram_fft(y, window, ws, n_fft, hop, n_mel, clip=1e-5, want_mag=False, kmax=0, lens=None, range_flag=None):
    """y [B,N] -> (mel [B,n_mel,F], energy [B,F], mag [B*F,516] or None) in one launch; range_flag: optional device int32 [1] the kernel
    raises when a sample leaves [-1, 1] (float bits of the largest |sample|)"""
    B, N = y.shape
    F = 1 + N // hop
    dev = y.device
    mel = torch.empty(B, n_mel, F, dtype=torch.float32, device=dev)
    energy = torch.empty(B, F, dtype=torch.float32, device=dev)
    mag = torch.empty(B * F, 516, dtype=torch.float32, device=dev) if want_mag else None
    lib = _lib.load()
    _lib.check(lib.ctts_mel_spectrogram(_p(_f32c(y, "y")), _p(lens), _p(_f32c(window, "window")), _p(ws), _p(mel), _p(energy), _p(mag), 516, B, N,
                                        int(n_fft), int(hop), int(n_mel), float(clip), int(kmax),
                                        None if range_flag is None else range_flag.data_ptr(),      # device or pinned host memory
                                        _stream()), "ctts_mel_spectrogram")
    return mel, energy, mag


# ---- HiFi-GAN vocoder (csrc/vocoder.hip) ------------------------------------------------------------------------------------
def vocoder_pack_weight(weight, transposed_u=0, planes=None, weight2=None):
    """Folded Conv1d weight [Cout, Cin, k] (transposed_u = 0) or ConvTranspose1d weight [Cin, Cout, k] (transposed_u = u) -> the packed
    operand of ctts_vocoder_conv: (w [roundup(N, 128), taps * roundup(Cin, 32)] fp32, w_planes or None).  `planes`: also split it
    (ctts_split_planes; None = the module default BF16_SPLIT).  Weight packing is a one-time layout change of a constant.
    `weight2` [Cout, Cin2, 1] (with a 1x1 Conv1d `weight` only): the two-operand form of vocoder_conv(..., x2=) -
    w [roundup(Cout, 128), roundup(Cin, 32) + roundup(Cin2, 32)], weight's columns first."""
    w = weight.detach().float()
    if weight2 is not None:
        w2 = weight2.detach().float()
        if transposed_u or w.dim() != 3 or w2.dim() != 3 or w.shape[2] != 1 or w2.shape[2] != 1 or w2.shape[0] != w.shape[0]:
            raise _lib.CttsError(f"vocoder_pack_weight: the two-operand form needs two 1x1 Conv1d weights of one Cout, got "
                                 f"{tuple(w.shape)} and {tuple(w2.shape)}")
        N, c1, c2 = w.shape[0], w.shape[1], w2.shape[1]
        npad, p1, p2 = -(-N // 128) * 128, -(-c1 // 32) * 32, -(-c2 // 32) * 32
        packed = torch.zeros(npad, p1 + p2, dtype=torch.float32, device=w.device)
        packed[:N, :c1] = w[:, :, 0]
        packed[:N, p1:p1 + c2] = w2[:, :, 0]
        use = BF16_SPLIT if planes is None else planes
        return packed, (split_planes([packed])[0] if use else None)
    if transposed_u:
        cin, cout, k = w.shape
        u = int(transposed_u)
        J = k // u
        # [Cin, Cout, J, u] (tap index r + j u) -> [u, Cout, J, Cin], taps reversed (tap' = J - 1 - j): column r Cout + co
        g = w.reshape(cin, cout, J, u).permute(3, 1, 2, 0).flip(2).reshape(u * cout, J, cin)
    else:
        g = w.permute(0, 2, 1)                         # [Cout, k, Cin]
    N, taps, cin = g.shape
    npad, cpad = -(-N // 128) * 128, -(-cin // 32) * 32
    packed = torch.zeros(npad, taps, cpad, dtype=torch.float32, device=w.device)
    packed[:N, :, :cin] = g
    packed = packed.reshape(npad, taps * cpad)
    use = BF16_SPLIT if planes is None else planes
    return packed, (split_planes([packed])[0] if use else None)


def _vocoder_lens(lens, len_mul, B, what):
    """the (pointer, multiplier) pair of a ragged vocoder launch: lens a device int32 [B] tensor (contiguous) or None = dense"""
    if lens is None:
        return None, 0
    if not (torch.is_tensor(lens) and lens.is_cuda and lens.dtype == torch.int32 and tuple(lens.shape) == (B,) and lens.is_contiguous()):
        raise _lib.CttsError(f"{what}: lens must be a contiguous device int32 tensor of shape ({B},)")
    if int(len_mul) < 1:
        raise _lib.CttsError(f"{what}: len_mul must be >= 1, got {len_mul}")
    return _p(lens), int(len_mul)


def _f16c(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float16 and t.is_contiguous()):
        raise _lib.CttsError(f"{name}: need a contiguous device float16 tensor")
    return t


def _vocoder_conv_desc(what, d, dtype, names, x, w, Cin, Cout, k, dil, transposed_u, slope, bias, R, out, alpha, beta, lens, len_mul,
                       Cin2=0):
    """What vocoder_conv and vocoder_conv_h share (`what`: the wrapper's name, for the messages; x already checked for dtype and rank):
    the shape, `out`, R, packed-weight and same-device checks, and the descriptor fields the two structs have in common.  `dtype` is
    the wrapper's type of w, R and out (float32 / float16), `names` its message names for them.  Cin2: the channels of vocoder_conv's
    second operand, which widen the packed weight.  -> out, allocated when not given."""
    act = _f32c if dtype == torch.float32 else _f16c
    B, T, cin = x.shape
    if cin != Cin:
        raise _lib.CttsError(f"{what}: x has {cin} channels, the layer {Cin}")
    Tout = T * transposed_u if transposed_u else T
    if out is None:
        if beta != 0.0:
            raise _lib.CttsError(f"{what}: beta != 0 needs `out`")
        out = torch.empty(B, Tout, Cout, dtype=dtype, device=x.device)
    elif tuple(out.shape) != (B, Tout, Cout):
        raise _lib.CttsError(f"{what}: out has shape {tuple(out.shape)}, expected {(B, Tout, Cout)}")
    if R is not None and tuple(R.shape) != (B, Tout, Cout):
        raise _lib.CttsError(f"{what}: R has shape {tuple(R.shape)}, expected {(B, Tout, Cout)}")
    N, taps = (transposed_u * Cout, k // transposed_u) if transposed_u else (Cout, k)
    wshape = (-(-N // 128) * 128, taps * (-(-Cin // 32) * 32) + -(-Cin2 // 32) * 32)
    if tuple(act(w, names[0]).shape) != wshape:
        raise _lib.CttsError(f"{what}: packed weight {tuple(w.shape)} does not match the layer (expected {wshape})")
    for t, name in ((w, "weight"), (bias, "bias"), (R, "R"), (out, "out")):
        if t is not None and t.device != x.device:
            raise _lib.CttsError(f"{what}: {name} is on {t.device}, x on {x.device}")
    d.x = _p(x)
    d.sxb, d.sxt, d.sxc = (int(s) for s in x.stride())
    d.B, d.T, d.Cin, d.Cout, d.k, d.dil = B, T, int(Cin), int(Cout), int(k), int(dil)
    d.transposed_u = int(transposed_u)
    d.act_in = 0 if slope is None else 1
    d.slope = 0.0 if slope is None else float(slope)
    d.w = _p(w)
    d.bias = _p(None if bias is None else _f32c(bias, "bias"))
    d.R = _p(None if R is None else act(R, names[1]))
    d.out = _p(act(out, names[2]))
    d.alpha, d.beta = float(alpha), float(beta)
    d.lens, d.len_mul = _vocoder_lens(lens, len_mul, B, what)
    return out


VOCODER_PAD_MODES = {"zero": 0, "reflect": 1}          # ctts_vconv_melgan_desc.pad_mode


def _vocoder_pad_mode(pad_mode, what):
    if pad_mode not in VOCODER_PAD_MODES:
        raise _lib.CttsError(f"{what}: pad_mode must be one of {tuple(VOCODER_PAD_MODES)}, got {pad_mode!r}")
    return VOCODER_PAD_MODES[pad_mode]


def vocoder_conv(x, w, w_planes, Cin, Cout, k, dil=1, transposed_u=0, slope=None, bias=None, R=None, out=None, alpha=1.0, beta=0.0,
                 bf16_split=None, lens=None, len_mul=1, pad_mode="zero", x2=None):
    """One generator layer (include/ctts.h ctts_vocoder_conv; with pad_mode="reflect" or x2, ctts_vocoder_conv_melgan).  x: [B, T, Cin] with any strides (fp32); w / w_planes from
    vocoder_pack_weight; slope: leaky_relu slope applied to x on load, or None.  -> out [B, T_out, Cout] (T_out = T or T u):
    out = beta * out + alpha * (conv + bias + R).  lens (device int32 [B]) / len_mul: the length-aware form - utterance b's input has
    min(lens[b] len_mul, T) rows, computed as a B = 1 call on them would; output rows beyond its end are left unwritten.
    MelGAN (include/ctts.h, MelGAN block): pad_mode="reflect" puts ReflectionPad1d(dil (k - 1) / 2) in place of the zero padding (Conv1d
    only, T above the padding), reflecting at each utterance's own end; x2 [B, T, Cin2] (k = 1 only, unit channel stride) is a second
    operand that is never activated: out = W [act(x) ; x2] + ..., w from vocoder_pack_weight(weight, weight2=)."""
    if x.dtype != torch.float32 or x.dim() != 3:
        raise _lib.CttsError(f"vocoder_conv: x must be a 3-D float32 tensor [B, T, Cin], got {x.dtype} {tuple(x.shape)}")
    split = BF16_SPLIT if bf16_split is None else int(bf16_split)
    if split and w_planes is None:
        raise _lib.CttsError("vocoder_conv: the split arithmetic needs w_planes")
    mode = _vocoder_pad_mode(pad_mode, "vocoder_conv")
    if mode and transposed_u:
        raise _lib.CttsError("vocoder_conv: pad_mode='reflect' is for Conv1d only (transposed_u must be 0)")
    if mode and x.shape[1] <= (k - 1) * dil // 2:
        raise _lib.CttsError(f"vocoder_conv: reflection needs T > dil (k - 1) / 2 = {(k - 1) * dil // 2}, got T = {x.shape[1]}")
    cin2 = 0
    if x2 is not None:
        if k != 1 or transposed_u:
            raise _lib.CttsError(f"vocoder_conv: x2 is for a 1x1 Conv1d only (k={k}, transposed_u={transposed_u})")
        if not (torch.is_tensor(x2) and x2.dtype == torch.float32 and x2.dim() == 3 and tuple(x2.shape[:2]) == tuple(x.shape[:2])
                and x2.stride(2) == 1 and x2.device == x.device):
            raise _lib.CttsError(f"vocoder_conv: x2 must be a float32 [B, T, Cin2] tensor on x's device with x's B and T and unit "
                                 f"channel stride, got {getattr(x2, 'dtype', type(x2))} {tuple(getattr(x2, 'shape', ()))}")
        cin2 = int(x2.shape[2])
    md = _lib.VconvMelganDesc() if mode or x2 is not None else None
    d = _lib.VconvDesc() if md is None else md.conv
    out = _vocoder_conv_desc("vocoder_conv", d, torch.float32, ("vocoder weight", "R", "out"), x, w, Cin, Cout, k, dil, transposed_u, slope,
                             bias, R, out, alpha, beta, lens, len_mul, Cin2=cin2)
    if split and w_planes.numel() != 3 * w.numel():          # w has the layer's shape by now: the planes are not its split
        raise _lib.CttsError(f"vocoder_conv: packed weight {tuple(w.shape)} does not match the layer (expected {tuple(w.shape)})")
    d.w_planes = _p(w_planes) if split else None
    d.bf16_split = split
    if md is None:
        _lib.check(_lib.load().ctts_vocoder_conv(C.byref(d), _stream()), "ctts_vocoder_conv")
        return out
    md.pad_mode = mode
    if x2 is not None:
        md.x2, md.sx2b, md.sx2t, md.Cin2 = _p(x2), int(x2.stride(0)), int(x2.stride(1)), cin2
    _lib.check(_lib.load().ctts_vocoder_conv_melgan(C.byref(md), _stream()), "ctts_vocoder_conv_melgan")
    return out


def vocoder_post(x, w, bias, slope=0.01, out=None, lens=None, len_mul=1, pad_mode="zero"):
    """conv_post + tanh (include/ctts.h ctts_vocoder_post): x [B, T, C] dense, w [k, C] (= weight[0].T), bias [1] -> [B, 1, T].
    lens (device int32 [B]) / len_mul: ctts_vocoder_post_ragged - out[b, 0, lens[b] len_mul:] = 0, rows there are never read.
    pad_mode="reflect": ctts_vocoder_post_reflect (MelGAN's ReflectionPad1d((k - 1) / 2) in front of the conv; dense or ragged)."""
    B, T, Cc = x.shape
    k = w.shape[0]
    if out is None:
        out = torch.empty(B, 1, T, dtype=torch.float32, device=x.device)
    if _vocoder_pad_mode(pad_mode, "vocoder_post"):
        lp, lm = _vocoder_lens(lens, len_mul, B, "vocoder_post")
        _lib.check(_lib.load().ctts_vocoder_post_reflect(_p(_f32c(x, "x")), B, T, Cc, int(k), _p(_f32c(w, "w")), _p(_f32c(bias, "bias")),
                                                         float(slope), _p(_f32c(out, "out")), lp, lm, _stream()),
                   "ctts_vocoder_post_reflect")
        return out
    if lens is not None:
        lp, lm = _vocoder_lens(lens, len_mul, B, "vocoder_post")
        _lib.check(_lib.load().ctts_vocoder_post_ragged(_p(_f32c(x, "x")), B, T, Cc, int(k), _p(_f32c(w, "w")), _p(_f32c(bias, "bias")),
                                                        float(slope), _p(_f32c(out, "out")), lp, lm, _stream()),
                   "ctts_vocoder_post_ragged")
        return out
    _lib.check(_lib.load().ctts_vocoder_post(_p(_f32c(x, "x")), B, T, Cc, int(k), _p(_f32c(w, "w")), _p(_f32c(bias, "bias")), float(slope),
                                             _p(_f32c(out, "out")), _stream()), "ctts_vocoder_post")
    return out


# ---- HiFi-GAN vocoder, fp16 mode (csrc/vocoder_h.hip) ---------------------------------------------------------------------------
FP16_MAX = 65504.0


def vocoder_pack_weight_h(weight, transposed_u=0):
    """Folded conv weight -> the packed fp16 operand of ctts_vocoder_conv_h [roundup(N, 128), taps * roundup(Cin, 32)]: the fp32 pack of
    vocoder_pack_weight, rounded once to fp16 (round to nearest even, saturated to +-65504).  A one-time layout change of a constant."""
    packed, _ = vocoder_pack_weight(weight, transposed_u, planes=False)
    return packed.clamp_(-FP16_MAX, FP16_MAX).to(torch.float16).contiguous()


def vocoder_conv_h(x, w, Cin, Cout, k, dil=1, transposed_u=0, slope=None, bias=None, R=None, out=None, alpha=1.0, beta=0.0,
                   lens=None, len_mul=1):
    """One generator layer in the fp16 mode (include/ctts.h ctts_vocoder_conv_h).  x: [B, T, Cin] with any strides, float32 (the mel:
    rounded to fp16 when staged) or float16; w from vocoder_pack_weight_h; bias fp32; R / out fp16 [B, T_out, Cout] dense.
    -> out = fp16(beta * out + alpha * (conv + bias + R)), saturated to +-65504.  lens / len_mul as vocoder_conv."""
    if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.float16) or x.dim() != 3:
        raise _lib.CttsError(f"vocoder_conv_h: x must be a 3-D float32 or float16 tensor [B, T, Cin], got "
                             f"{getattr(x, 'dtype', type(x))} {tuple(getattr(x, 'shape', ()))}")
    if not x.is_cuda:
        raise _lib.CttsError("vocoder_conv_h: x must be a device (HIP) tensor")
    d = _lib.VconvHDesc()
    out = _vocoder_conv_desc("vocoder_conv_h", d, torch.float16, ("vocoder_conv_h weight", "vocoder_conv_h R", "vocoder_conv_h out"), x, w, Cin,
                             Cout, k, dil, transposed_u, slope, bias, R, out, alpha, beta, lens, len_mul)
    d.x_f32 = 1 if x.dtype == torch.float32 else 0
    _lib.check(_lib.load().ctts_vocoder_conv_h(C.byref(d), _stream()), "ctts_vocoder_conv_h")
    return out


def vocoder_post_h(x, w, bias, slope=0.01, out=None, lens=None, len_mul=1):
    """conv_post + tanh on fp16 activations (include/ctts.h ctts_vocoder_post_h): x fp16 [B, T, C] dense, w fp32 [k, C], bias fp32 [1]
    -> fp32 [B, 1, T]; lens (device int32 [B]) / len_mul: exact zeros from row lens[b] len_mul on."""
    if not torch.is_tensor(x) or x.dim() != 3:
        raise _lib.CttsError("vocoder_post_h: x must be a 3-D float16 tensor [B, T, C]")
    _f16c(x, "vocoder_post_h x")
    B, T, Cc = x.shape
    if w.dim() != 2 or w.shape[1] != Cc or w.shape[0] % 2 == 0:
        raise _lib.CttsError(f"vocoder_post_h: w must be [k, {Cc}] with k odd, got {tuple(w.shape)}")
    k = w.shape[0]
    if out is None:
        out = torch.empty(B, 1, T, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (B, 1, T):
        raise _lib.CttsError(f"vocoder_post_h: out has shape {tuple(out.shape)}, expected {(B, 1, T)}")
    lp, lm = _vocoder_lens(lens, len_mul, B, "vocoder_post_h")
    _lib.check(_lib.load().ctts_vocoder_post_h(_p(x), B, T, Cc, int(k), _p(_f32c(w, "w")), _p(_f32c(bias, "bias")), float(slope),
                                               _p(_f32c(out, "out")), lp, lm, _stream()), "ctts_vocoder_post_h")
    return out


# ---- Fastformer additive attention (csrc/fastformer.hip) ----------------------------------------------------------------------
def _rows_ld(t, C, name):
    """(row stride) of a [B*T, C]-shaped fp32 operand that may be a column slice of a wider matrix (unit column stride)"""
    if t.dtype != torch.float32 or t.stride(-1) != 1 or t.dim() < 2:
        raise _lib.CttsError(f"{name}: need a float32 matrix with unit column stride, got {t.dtype} {tuple(t.shape)} {t.stride()}")
    ld = t.stride(-2)
    if t.dim() == 3 and t.stride(0) != ld * t.shape[1]:
        raise _lib.CttsError(f"{name}: batch stride {t.stride(0)} is not T * row stride")
    return ld


def fastformer_workspace(B, T, H, Cc, device):
    n = _lib.load().ctts_fastformer_workspace_floats(int(B), int(T), int(H), int(Cc))
    return torch.empty(max(int(n), 1), dtype=torch.float32, device=device)


def fastformer_pool_fwd(s, V, lens, B, T, H, div):
    """alpha = softmax_t(s / div + (t < lens[b] ? -10000 : 0)) per (b, h);  p[b, c] = sum_t alpha[b, t, c // D] V[b, t, c].
    s: [B*T, H] logits (row stride may exceed H), V: [B*T, C] values -> (p [B, C], stats [B, H, 2])"""
    Cc = V.shape[-1]
    p = torch.empty(B, Cc, dtype=torch.float32, device=V.device)
    stats = torch.empty(B, H, 2, dtype=torch.float32, device=V.device)
    ws = fastformer_workspace(B, T, H, Cc, V.device)
    _lib.check(_lib.load().ctts_fastformer_pool_fwd(_p(s), _rows_ld(s, H, "s"), _p(V), _rows_ld(V, Cc, "V"), _p(lens), _p(p), _p(stats),
                                                    _p(ws), int(B), int(T), int(H), int(Cc), float(div), _stream()), "ctts_fastformer_pool_fwd")
    return p, stats


def fastformer_pool_bwd(dp, p, stats, s, V, lens, B, T, H, div, dV_in=None):
    """-> (dV [B*T, C] = dV_in + alpha dp,  ds [B*T, H]); dV is written into dV_in when it is given"""
    Cc = V.shape[-1]
    dV = dV_in if dV_in is not None else torch.empty(B * T, Cc, dtype=torch.float32, device=V.device)
    ds = torch.empty(B * T, H, dtype=torch.float32, device=V.device)
    _lib.check(_lib.load().ctts_fastformer_pool_bwd(_p(_f32c(dp, "dp")), _p(_f32c(p, "p")), _p(_f32c(stats, "stats")), _p(s),
                                                    _rows_ld(s, H, "s"), _p(V), _rows_ld(V, Cc, "V"), _p(lens),
                                                    _p(None if dV_in is None else _f32c(dV_in, "dV_in")), _p(dV), _p(ds), int(B), int(T),
                                                    int(H), int(Cc), float(div), _stream()), "ctts_fastformer_pool_bwd")
    return dV, ds


def fastformer_bcast(X, p, B, T):
    """Y [B*T, C] = X[b, t, :] * p[b, :]"""
    Cc = X.shape[-1]
    Y = torch.empty(B * T, Cc, dtype=torch.float32, device=X.device)
    _lib.check(_lib.load().ctts_fastformer_bcast(_p(X), _rows_ld(X, Cc, "X"), _p(_f32c(p, "p")), _p(Y), int(B), int(T), int(Cc), _stream()),
               "ctts_fastformer_bcast")
    return Y


def fastformer_bcast_bwd(dY1, X, p, B, T, dY2=None, dX_in=None, out=None):
    """dy = dY1 + dY2 -> (dX = dX_in + dy * p[b],  dp [B, C] = sum_t dy * X); dX goes to `out` (may be dX_in) or a new tensor"""
    Cc = X.shape[-1]
    dX = out if out is not None else torch.empty(B * T, Cc, dtype=torch.float32, device=X.device)
    dp = torch.empty(B, Cc, dtype=torch.float32, device=X.device)
    ws = fastformer_workspace(B, T, 0, Cc, X.device)
    _lib.check(_lib.load().ctts_fastformer_bcast_bwd(_p(_f32c(dY1, "dY1")), _p(None if dY2 is None else _f32c(dY2, "dY2")), _p(X),
                                                     _rows_ld(X, Cc, "X"), _p(_f32c(p, "p")),
                                                     _p(None if dX_in is None else _f32c(dX_in, "dX_in")), _p(dX), _p(dp), _p(ws), int(B),
                                                     int(T), int(Cc), _stream()), "ctts_fastformer_bcast_bwd")
    return dX, dp


def fastformer_resdrop(x, t, rowscale=None, p_drop=0.0, seed=None, drop_offset=0):
    """y = rowscale * (x + dropout(t))"""
    Cc = t.shape[-1]
    y = torch.empty_like(t)
    _lib.check(_lib.load().ctts_fastformer_resdrop(_p(_f32c(x, "x")), _p(_f32c(t, "t")), _p(y), None, t.numel() // Cc, int(Cc), _p(rowscale),
                                                   float(p_drop), _p(seed), int(drop_offset), 0, _stream()), "ctts_fastformer_resdrop")
    return y


def fastformer_resdrop_bwd(dy, rowscale=None, p_drop=0.0, seed=None, drop_offset=0):
    """-> (dx = rowscale * dy,  dt = rowscale * dropout(dy))"""
    Cc = dy.shape[-1]
    dt, dx = torch.empty_like(dy), torch.empty_like(dy)
    _lib.check(_lib.load().ctts_fastformer_resdrop(None, _p(_f32c(dy, "dy")), _p(dt), _p(dx), dy.numel() // Cc, int(Cc), _p(rowscale),
                                                   float(p_drop), _p(seed), int(drop_offset), 1, _stream()), "ctts_fastformer_resdrop")
    return dx, dt


# ---- Griffin-Lim / STFT (csrc/griffinlim.hip) ---------------------------------------------------------------------------------
GL_NFFT, GL_HOP, GL_NBINS = 1024, 256, 513


def griffinlim_prepare(window):
    """window [1024] float32 (device) -> workspace of the STFT / Griffin-Lim kernels (twiddles, window, window^2)"""
    lib = _lib.load()
    ws = torch.empty(lib.ctts_griffinlim_workspace_bytes(GL_NFFT, GL_HOP) // 4, dtype=torch.float32, device=window.device)
    _lib.check(lib.ctts_griffinlim_prepare(_p(_f32c(window, "window")), GL_NFFT, GL_HOP, _p(ws), _stream()), "ctts_griffinlim_prepare")
    return ws


def _frames_arg(frames):
    if frames is None:
        return None
    if not frames.is_cuda or frames.dtype != torch.int32 or not frames.is_contiguous():
        raise _lib.CttsError("frames / lens: expected a contiguous int32 device tensor")
    return frames


def stft_transform(x, ws, lens=None):
    """x [B,N] float32 -> (magnitude, phase) [B,513,F], F = 1 + N // 256 (STFT.transform, audio/stft.py:59-88); lens: int32 [B] samples"""
    B, N = x.shape
    F = 1 + N // GL_HOP
    mag = torch.empty(B, GL_NBINS, F, dtype=torch.float32, device=x.device)
    phase = torch.empty_like(mag)
    lib = _lib.load()
    _lib.check(lib.ctts_stft_transform(_p(_f32c(x, "x")), _p(_frames_arg(lens)), _p(ws), _p(mag), _p(phase), GL_NBINS * F, F, 1,
                                       B, N, GL_NFFT, GL_HOP, _stream()), "ctts_stft_transform")
    return mag, phase


def istft_frames(mag, phase, ws, frames=None, want_magT=False):
    """(mag, phase) [B,513,F] contiguous -> (Y [B,F,1024] windowed inverse-DFT frames, frame-major magnitude copy [B,F,513] or None)"""
    B, nb, F = mag.shape
    if nb != GL_NBINS or phase.shape != mag.shape:
        raise _lib.CttsError(f"istft_frames: expected magnitude and phase [B, 513, F], got {tuple(mag.shape)} / {tuple(phase.shape)}")
    Y = torch.empty(B, F, GL_NFFT, dtype=torch.float32, device=mag.device)
    magT = torch.empty(B, F, GL_NBINS, dtype=torch.float32, device=mag.device) if want_magT else None
    lib = _lib.load()
    _lib.check(lib.ctts_istft_frames(_p(_f32c(mag, "magnitude")), _p(_f32c(phase, "phase")), GL_NBINS * F, F, 1, _p(_frames_arg(frames)),
                                     _p(ws), _p(Y), _p(magT), B, F, GL_NFFT, GL_HOP, _stream()), "ctts_istft_frames")
    return Y, magT


def griffinlim_iter(Y_in, magT, ws, Y_out, frames=None):
    """one Griffin-Lim iteration on the frame buffers (Y_in -> Y_out, [B,F,1024]); magT [B,F,513] the target magnitude"""
    B, F, _ = Y_in.shape
    lib = _lib.load()
    _lib.check(lib.ctts_griffinlim_iter(_p(_f32c(Y_in, "Y_in")), _p(_f32c(magT, "magT")), _p(_frames_arg(frames)), _p(ws),
                                        _p(_f32c(Y_out, "Y_out")), B, F, GL_NFFT, GL_HOP, _stream()), "ctts_griffinlim_iter")
    return Y_out


def griffinlim_state(B, F, device):
    """the state buffer of griffinlim_iter_momentum for frame buffers [B,F,1024]: one slot per frame (the previous rebuilt spectrum),
    uninitialised - the first iteration (first=True) only writes it"""
    return torch.empty(_lib.load().ctts_griffinlim_state_floats(int(B), int(F)), dtype=torch.float32, device=device)


def griffinlim_iter_momentum(Y_in, magT, state, ws, Y_out, coef, first, frames=None):
    """one fast Griffin-Lim iteration (Y_in -> Y_out, [B,F,1024]): A = X - coef T_prev, T_prev <- X in `state` (griffinlim_state), A
    rescaled to magT [B,F,513]; coef = momentum / (1 + momentum); first: the state counts as zero and is only written"""
    B, F, _ = Y_in.shape
    lib = _lib.load()
    if not state.is_cuda or state.dtype != torch.float32 or not state.is_contiguous() or state.numel() < lib.ctts_griffinlim_state_floats(B, F):
        raise _lib.CttsError(f"griffinlim_iter_momentum: state must be a contiguous float32 device tensor of griffinlim_state({B}, {F})")
    _lib.check(lib.ctts_griffinlim_iter_momentum(_p(_f32c(Y_in, "Y_in")), _p(_f32c(magT, "magT")), _p(state), _p(_frames_arg(frames)), _p(ws),
                                                 _p(_f32c(Y_out, "Y_out")), float(coef), int(bool(first)), B, F, GL_NFFT, GL_HOP, _stream()),
               "ctts_griffinlim_iter_momentum")
    return Y_out


def istft_frames_seeded(mag, ws, seed, frames=None, want_magT=False):
    """istft_frames with the initial phase drawn on the device: theta(b, k, f) = 2 pi u(seed, b, k, f).  mag [B,513,F] contiguous,
    seed a one-element int64 device tensor (read by the kernel) -> (Y [B,F,1024], frame-major magnitude copy [B,F,513] or None)"""
    B, nb, F = mag.shape
    if nb != GL_NBINS:
        raise _lib.CttsError(f"istft_frames_seeded: expected magnitude [B, 513, F], got {tuple(mag.shape)}")
    if not torch.is_tensor(seed) or not seed.is_cuda or seed.dtype != torch.int64 or seed.numel() != 1:
        raise _lib.CttsError("istft_frames_seeded: seed must be a one-element int64 device tensor")
    Y = torch.empty(B, F, GL_NFFT, dtype=torch.float32, device=mag.device)
    magT = torch.empty(B, F, GL_NBINS, dtype=torch.float32, device=mag.device) if want_magT else None
    lib = _lib.load()
    _lib.check(lib.ctts_istft_frames_seeded(_p(_f32c(mag, "magnitude")), GL_NBINS * F, F, 1, _p(_frames_arg(frames)), _p(ws), _p(seed),
                                            _p(Y), _p(magT), B, F, GL_NFFT, GL_HOP, _stream()), "ctts_istft_frames_seeded")
    return Y, magT


def istft_ola(Y, ws, frames=None, out=None):
    """Y [B,F,1024] -> waveform [B, 256 (F - 1)] (overlap-add, window-sum division, * 4, crop)"""
    B, F, _ = Y.shape
    L = GL_HOP * (F - 1)
    if out is None:
        out = torch.empty(B, L, dtype=torch.float32, device=Y.device)
    lib = _lib.load()
    _lib.check(lib.ctts_istft_ola(_p(_f32c(Y, "Y")), _p(_frames_arg(frames)), _p(ws), _p(_f32c(out, "out")), out.shape[-1], B, F,
                                  GL_NFFT, GL_HOP, _stream()), "ctts_istft_ola")
    return out


# ---- pitch targets: F0 tracker and the F0 -> continuous log-F0 -> CWT chain (csrc/pitchtrack.hip) -----------------------------
F0T_MAX_FRAMES, F0T_NSCALE = 4096, 10


def _al4(t, name):
    if t.data_ptr() % 4:
        raise _lib.CttsError(f"{name}: the data pointer must be 4-byte aligned")
    return t


def pitch_track_prepare(device):
    """-> workspace tensor of `pitch_track` (FFT twiddles, hann window and the window's normalised autocorrelation)"""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.CttsError("pitch_track_prepare: needs a HIP device - no CPU fallback exists")
    lib = _lib.load()
    ws = torch.empty(lib.ctts_pitch_track_workspace_bytes() // 4, dtype=torch.float32, device=device)
    _lib.check(lib.ctts_pitch_track_prepare(_p(ws), _stream()), "ctts_pitch_track_prepare")
    return ws


def pitch_track(wav, ws, lens=None, sr=22050, hop=256, f0_min=80.0, f0_max=750.0, voicing_threshold=0.6, silence_threshold=0.03):
    """wav [B,N] float32, lens int32 [B] samples or None -> (f0 [B,F] Hz, 0 = unvoiced; strength [B,F]), F = 1 + N // hop"""
    if not torch.is_tensor(wav) or wav.dim() != 2:
        raise _lib.CttsError("pitch_track: expected wav [B, N]")
    B, N = wav.shape
    if B < 1 or N < 1:
        raise _lib.CttsError(f"pitch_track: empty batch {tuple(wav.shape)}")
    _p(wav)                                                # CPU tensor -> CttsError
    _al4(_f32c(wav, "wav"), "wav")
    if lens is not None and (_frames_arg(lens).numel() != B):
        raise _lib.CttsError(f"pitch_track: {lens.numel()} lengths for a batch of {B}")
    if int(hop) < 1:
        raise _lib.CttsError(f"pitch_track: hop must be >= 1, got {hop}")
    F = 1 + N // int(hop)
    f0 = torch.empty(B, F, dtype=torch.float32, device=wav.device)
    strength = torch.empty_like(f0)
    peak = torch.empty(B * 32, dtype=torch.float32, device=wav.device)          # scratch: the utterance peaks, 32 slices each
    _lib.check(_lib.load().ctts_pitch_track(_p(wav), _p(lens), _p(_f32c(ws, "workspace")), _p(peak), _p(f0), _p(strength), B, N, int(sr), int(hop),
                                            float(f0_min), float(f0_max), float(voicing_threshold), float(silence_threshold), _stream()),
               "ctts_pitch_track")
    return f0, strength


def _f0_frames_args(f0, frames, what):
    if not torch.is_tensor(f0) or f0.dim() != 2:
        raise _lib.CttsError(f"{what}: expected f0 [B, F]")
    _p(f0)
    _al4(_f32c(f0, "f0"), "f0")
    B, F = f0.shape
    if B < 1 or F < 1:
        raise _lib.CttsError(f"{what}: empty batch {tuple(f0.shape)}")
    if frames is None or not torch.is_tensor(frames) or _frames_arg(frames).numel() != B:
        raise _lib.CttsError(f"{what}: frames must be an int32 device tensor with one entry per utterance")
    return B, F


def f0_targets(f0, frames):
    """f0 [B,F] Hz (0 = unvoiced), frames int32 [B] -> (uv [B,F], cont_lf0 [B,F], mean_std [B,2], cwt_spec [B,F,10], valid int32 [B])"""
    B, F = _f0_frames_args(f0, frames, "f0_targets")
    dev = f0.device
    uv = torch.empty(B, F, dtype=torch.float32, device=dev)
    cont = torch.empty_like(uv)
    mean_std = torch.empty(B, 2, dtype=torch.float32, device=dev)
    cwt = torch.empty(B, F, F0T_NSCALE, dtype=torch.float32, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().ctts_f0_targets(_p(f0), _p(frames), _p(uv), _p(cont), _p(mean_std), _p(cwt), _p(valid), B, F, _stream()), "ctts_f0_targets")
    return uv, cont, mean_std, cwt, valid


def norm_interp_f0(f0, frames, eps=1e-9):
    """f0 [B,F] Hz, frames int32 [B] -> (log2 f0 interpolated over the unvoiced frames [B,F], uv [B,F])"""
    B, F = _f0_frames_args(f0, frames, "norm_interp_f0")
    out = torch.empty(B, F, dtype=torch.float32, device=f0.device)
    uv = torch.empty_like(out)
    _lib.check(_lib.load().ctts_norm_interp_f0(_p(f0), _p(frames), _p(out), _p(uv), B, F, float(eps), _stream()), "ctts_norm_interp_f0")
    return out, uv


# ---- dataset preparation: silence trim, alignment prior, outlier filter + moments (csrc/preprocess.hip) ---------------------------
OUTLIER_MAX_VALUES = 4096


def _lens_i32(lens, B, what):
    if lens is None or not torch.is_tensor(lens) or _frames_arg(lens).numel() != B:
        raise _lib.CttsError(f"{what}: lengths must be an int32 device tensor with one entry per utterance")
    return lens


def trim_silence(wav, lens, top_db, frame_length=1024, hop=256):
    """wav [B,N] float32, lens int32 [B] samples -> (start int32 [B], end int32 [B], mse [B, 1 + N // hop] - the frame powers)"""
    if not torch.is_tensor(wav) or wav.dim() != 2:
        raise _lib.CttsError("trim_silence: expected wav [B, N]")
    _p(wav)
    _al4(_f32c(wav, "wav"), "wav")
    B, N = wav.shape
    if B < 1 or N < 1:
        raise _lib.CttsError(f"trim_silence: empty batch {tuple(wav.shape)}")
    _lens_i32(lens, B, "trim_silence")
    if int(hop) < 1 or int(frame_length) < 2:
        raise _lib.CttsError(f"trim_silence: need frame_length >= 2 and hop >= 1, got {frame_length} / {hop}")
    lib = _lib.load()
    mse = torch.empty(lib.ctts_trim_silence_workspace_bytes(B, N, int(hop)) // 4, dtype=torch.float32, device=wav.device)
    start = torch.empty(B, dtype=torch.int32, device=wav.device)
    end = torch.empty_like(start)
    _lib.check(lib.ctts_trim_silence(_p(wav), _p(lens), _p(mse), _p(start), _p(end), B, N, float(top_db), int(frame_length), int(hop), _stream()),
               "ctts_trim_silence")
    return start, end, mse.view(B, 1 + N // int(hop))


def attn_prior(src_lens, mel_lens, out, scaling_factor=1.0):
    """src_lens, mel_lens int32 [B]; out float32 [B,Ts,Tm] view with a contiguous last dimension - written in place, every element"""
    if not torch.is_tensor(out) or out.dim() != 3 or out.dtype != torch.float32:
        raise _lib.CttsError("attn_prior: out must be a float32 [B, Ts, Tm] tensor")
    _p(out)
    _al4(out, "out")
    B, Ts, Tm = out.shape
    if B < 1 or Ts < 1 or Tm < 1:
        raise _lib.CttsError(f"attn_prior: empty output {tuple(out.shape)}")
    sb, ss, st = out.stride()
    if st != 1 and Tm > 1:
        raise _lib.CttsError("attn_prior: the last dimension of out must be contiguous")
    if Ts == 1:
        ss = max(ss, Tm)
    if B == 1:
        sb = max(sb, (Ts - 1) * ss + Tm)
    _lens_i32(src_lens, B, "attn_prior")
    _lens_i32(mel_lens, B, "attn_prior")
    _lib.check(_lib.load().ctts_attn_prior(_p(src_lens), _p(mel_lens), _p(out), B, Ts, Tm, sb, ss, float(scaling_factor), _stream()), "ctts_attn_prior")
    return out


def outlier_stats(values, lens):
    """values [B,L] float32, lens int32 [B] -> (keep uint8 [B,L], count int32 [B], sum float64 [B], m2 float64 [B], min [B], max [B])"""
    if not torch.is_tensor(values) or values.dim() != 2:
        raise _lib.CttsError("outlier_stats: expected values [B, L]")
    _p(values)
    _al4(_f32c(values, "values"), "values")
    B, L = values.shape
    if B < 1 or L < 1:
        raise _lib.CttsError(f"outlier_stats: empty batch {tuple(values.shape)}")
    _lens_i32(lens, B, "outlier_stats")
    dev = values.device
    keep = torch.empty(B, L, dtype=torch.uint8, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    s = torch.empty(B, dtype=torch.float64, device=dev)
    m2 = torch.empty_like(s)
    lo = torch.empty(B, dtype=torch.float32, device=dev)
    hi = torch.empty_like(lo)
    _lib.check(_lib.load().ctts_outlier_stats(_p(values), _p(lens), _p(keep), _p(count), _p(s), _p(m2), _p(lo), _p(hi), B, L, _stream()),
               "ctts_outlier_stats")
    return keep, count, s, m2, lo, hi


# ---- objective evaluation: mel cepstrum, DTW, path metrics (csrc/metrics.hip) -------------------------------------------------------
CEPSTRUM_MAX_COEF = 32
DTW_MAX_FRAMES = 2048
DTW_ALIGN = {"dtw": 0, "none": 1}


def mel_cepstrum(mel, frames=None, n_coef=13):
    """mel [B,n_mel,F] float32 (natural-log mel), frames int32 [B] or None -> cepstra [B,F,n_coef] (DCT-II coefficients 1 .. n_coef)"""
    if not torch.is_tensor(mel) or mel.dim() != 3:
        raise _lib.CttsError("mel_cepstrum: expected mel [B, n_mel, F]")
    _p(mel)
    _al4(_f32c(mel, "mel"), "mel")
    B, M, F = mel.shape
    n_coef = int(n_coef)
    if B < 1 or F < 1:
        raise _lib.CttsError(f"mel_cepstrum: empty batch {tuple(mel.shape)}")
    if not (1 <= n_coef <= CEPSTRUM_MAX_COEF and n_coef < M):
        raise _lib.CttsError(f"mel_cepstrum: need 1 <= n_coef <= {CEPSTRUM_MAX_COEF} and n_coef < n_mel = {M}, got {n_coef}")
    if frames is not None:
        _lens_i32(frames, B, "mel_cepstrum")
    out = torch.empty(B, F, n_coef, dtype=torch.float32, device=mel.device)
    _lib.check(_lib.load().ctts_mel_cepstrum(_p(mel), _p(frames), _p(out), B, M, F, n_coef, _stream()), "ctts_mel_cepstrum")
    return out


def dtw(x, x_lens, y, y_lens, align="dtw"):
    """x [B,Tx,K], y [B,Ty,K] float32, x_lens / y_lens int32 [B] -> (cost [B], path_len int32 [B], path int32 [B, Tx + Ty - 1, 2]);
    align "dtw" or "none" (frame i against frame i).  Padded Tx, Ty <= 2048: refused before any launch otherwise."""
    if not torch.is_tensor(x) or not torch.is_tensor(y) or x.dim() != 3 or y.dim() != 3:
        raise _lib.CttsError("dtw: expected x [B, Tx, K] and y [B, Ty, K]")
    _p(x), _p(y)
    _al4(_f32c(x, "x"), "x"), _al4(_f32c(y, "y"), "y")
    if align not in DTW_ALIGN:
        raise _lib.CttsError(f"dtw: align {align!r}: expected 'dtw' or 'none'")
    B, Tx, K = x.shape
    Ty = y.shape[1]
    if y.shape[0] != B or y.shape[2] != K:
        raise _lib.CttsError(f"dtw: x {tuple(x.shape)} against y {tuple(y.shape)}")
    if B < 1 or Tx < 1 or Ty < 1:
        raise _lib.CttsError(f"dtw: empty batch {tuple(x.shape)} / {tuple(y.shape)}")
    if Tx > DTW_MAX_FRAMES or Ty > DTW_MAX_FRAMES:
        raise _lib.CttsError(f"dtw: padded lengths {Tx} x {Ty} exceed {DTW_MAX_FRAMES} frames per side")
    if not 1 <= K <= CEPSTRUM_MAX_COEF:
        raise _lib.CttsError(f"dtw: K = {K} outside [1, {CEPSTRUM_MAX_COEF}]")
    _lens_i32(x_lens, B, "dtw")
    _lens_i32(y_lens, B, "dtw")
    dev = x.device
    lib = _lib.load()
    ws = torch.empty(lib.ctts_dtw_workspace_bytes(B, Tx, Ty) // 4, dtype=torch.int32, device=dev) if align == "dtw" else None
    cost = torch.empty(B, dtype=torch.float32, device=dev)
    path_len = torch.empty(B, dtype=torch.int32, device=dev)
    path = torch.empty(B, Tx + Ty - 1, 2, dtype=torch.int32, device=dev)
    _lib.check(lib.ctts_dtw(_p(x), _p(y), _p(x_lens), _p(y_lens), _p(ws), _p(cost), _p(path_len), _p(path), B, Tx, Ty, K, DTW_ALIGN[align],
                            _stream()), "ctts_dtw")
    return cost, path_len, path


def path_metrics(path, path_len, f0_x, f0_y):
    """path int32 [B,P,2], path_len int32 [B], f0_x [B,Tx], f0_y [B,Ty] Hz (0 = unvoiced) -> float64 [B,4]: pairs, pairs voiced in both,
    sum of squared log-F0 differences in cents over those, pairs whose voicing differs"""
    if not torch.is_tensor(path) or path.dim() != 3 or path.shape[2] != 2:
        raise _lib.CttsError("path_metrics: expected path [B, P, 2]")
    _p(path)
    if path.dtype != torch.int32 or not path.is_contiguous():
        raise _lib.CttsError("path_metrics: path must be a contiguous int32 tensor")
    B, P, _ = path.shape
    if B < 1 or P < 1:
        raise _lib.CttsError(f"path_metrics: empty path {tuple(path.shape)}")
    _lens_i32(path_len, B, "path_metrics")
    for t, name in ((f0_x, "f0_x"), (f0_y, "f0_y")):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] != B or t.shape[1] < 1:
            raise _lib.CttsError(f"path_metrics: expected {name} [B, T] with B = {B}")
        _p(t)
        _al4(_f32c(t, name), name)
    out = torch.empty(B, 4, dtype=torch.float64, device=path.device)
    _lib.check(_lib.load().ctts_path_metrics(_p(path), _p(path_len), _p(f0_x), _p(f0_y), _p(out), B, f0_x.shape[1], f0_y.shape[1], P, _stream()),
               "ctts_path_metrics")
    return out


# ---- audio resampling and peak normalisation (csrc/resample.hip) -------------------------------------------------------------------
RESAMPLE_MAX_RATIO_TERM = 1024        # L, M after reduction
RESAMPLE_MAX_PHASE_TAPS = 1024        # T
RESAMPLE_TAP_GRANULE = 8              # T is a multiple of this: the kernel loads eight coefficients at a time
RESAMPLE_MAX_SAMPLES = 1 << 30        # per row, on either side


def resample_tile(L, M, T, half):
    """Consecutive outputs one tile of the resampling kernel covers for these parameters (a multiple of L; 0 for L == M or parameters
    the kernel refuses).  It depends on (L, M, T, half) alone."""
    return int(_lib.load().ctts_resample_tile(int(L), int(M), int(T), int(half)))


def resample(wav, lens, bank, L, M, half):
    """wav [B,N] float32, lens int32 [B], bank [L,T] float32 (None when L == M) -> (out [B, ceil(N L / M)], out_lens int32 [B]):
    out[b][n] = sum_j bank[(n M + half) mod L][j] wav[b][(n M + half) div L - j] over the row's own lens[b] samples"""
    if not torch.is_tensor(wav) or wav.dim() != 2:
        raise _lib.CttsError("resample: expected wav [B, N]")
    _p(wav)
    _al4(_f32c(wav, "wav"), "wav")
    B, N = wav.shape
    L, M, half = int(L), int(M), int(half)
    if B < 1 or N < 1:
        raise _lib.CttsError(f"resample: empty batch {tuple(wav.shape)}")
    if B > 65535:
        raise _lib.CttsError(f"resample: at most 65535 utterances per call, got {B}")
    if not (1 <= L <= RESAMPLE_MAX_RATIO_TERM and 1 <= M <= RESAMPLE_MAX_RATIO_TERM):
        raise _lib.CttsError(f"resample: the reduced ratio {L}/{M} has a term outside [1, {RESAMPLE_MAX_RATIO_TERM}]")
    No = (N * L + M - 1) // M
    if N > RESAMPLE_MAX_SAMPLES or No > RESAMPLE_MAX_SAMPLES:
        raise _lib.CttsError(f"resample: {N} -> {No} samples per row exceed 2^30")
    _lens_i32(lens, B, "resample")
    T = 0
    if L != M:
        if not torch.is_tensor(bank) or bank.dim() != 2 or bank.shape[0] != L:
            raise _lib.CttsError(f"resample: expected bank [L = {L}, T]")
        _p(bank)
        _f32c(bank, "bank")
        T = bank.shape[1]
        if T % RESAMPLE_TAP_GRANULE or not RESAMPLE_TAP_GRANULE <= T <= RESAMPLE_MAX_PHASE_TAPS:
            raise _lib.CttsError(f"resample: T = {T} must be a multiple of {RESAMPLE_TAP_GRANULE} in [{RESAMPLE_TAP_GRANULE}, {RESAMPLE_MAX_PHASE_TAPS}]")
        if half < 0 or 2 * half + 1 > L * T:
            raise _lib.CttsError(f"resample: a bank [{L}, {T}] does not hold 2 * {half} + 1 taps")
        if bank.data_ptr() % 32:
            raise _lib.CttsError("resample: bank must be 32-byte aligned")
    out = torch.empty(B, No, dtype=torch.float32, device=wav.device)
    out_lens = torch.empty(B, dtype=torch.int32, device=wav.device)
    _lib.check(_lib.load().ctts_resample(_p(wav), _p(lens), _p(bank) if L != M else None, _p(out), _p(out_lens), B, N, L, M, T, half, _stream()),
               "ctts_resample")
    return out, out_lens


def peak_normalize(wav, lens, max_wav_value=32768.0, return_int16=False):
    """wav [B,N] float32, lens int32 [B] -> (out float32 [B,N] = trunc(wav / peak * max_wav_value) saturated to int16, over 32768;
    int16 [B,N] or None; peak [B]; valid int32 [B])"""
    if not torch.is_tensor(wav) or wav.dim() != 2:
        raise _lib.CttsError("peak_normalize: expected wav [B, N]")
    _p(wav)
    _al4(_f32c(wav, "wav"), "wav")
    B, N = wav.shape
    if B < 1 or N < 1:
        raise _lib.CttsError(f"peak_normalize: empty batch {tuple(wav.shape)}")
    if B > 65535:
        raise _lib.CttsError(f"peak_normalize: at most 65535 utterances per call, got {B}")
    mwv = float(max_wav_value)
    if not (0.0 < mwv < float("inf")):
        raise _lib.CttsError(f"peak_normalize: max_wav_value must be positive and finite, got {max_wav_value}")
    _lens_i32(lens, B, "peak_normalize")
    dev = wav.device
    out = torch.empty_like(wav)
    q16 = torch.empty(B, N, dtype=torch.int16, device=dev) if return_int16 else None
    peak = torch.empty(B, dtype=torch.float32, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().ctts_peak_normalize(_p(wav), _p(lens), _p(out), _p(q16), _p(peak), _p(valid), B, N, mwv, _stream()),
               "ctts_peak_normalize")
    return out, q16, peak, valid


# ---- loudness metering and normalisation (csrc/loudness.hip) -----------------------------------------------------------------------
LOUDNESS_MAX_SAMPLES = 1 << 24        # per row


def loudness_chunk():
    """samples one lane of the K-weighting kernels filters: utterances are chained in chunks of this many samples from their sample 0"""
    return int(_lib.load().ctts_loudness_chunk())


def loudness_limits():
    """-> (hop segments a 64-chunk tile may touch, float64 words of the coefficient buffer, blocks / segments the gate holds)"""
    lib = _lib.load()
    return int(lib.ctts_loudness_tile_slots()), int(lib.ctts_loudness_coef_doubles()), int(lib.ctts_loudness_max_segments())


def _loudness_batch(wav, lens, what):
    if not torch.is_tensor(wav) or wav.dim() != 2:
        raise _lib.CttsError(f"{what}: expected wav [B, N]")
    _p(wav)
    _al4(_f32c(wav, "wav"), "wav")
    B, N = wav.shape
    if B < 1 or N < 1:
        raise _lib.CttsError(f"{what}: empty batch {tuple(wav.shape)}")
    if B > 65535 or N > LOUDNESS_MAX_SAMPLES:
        raise _lib.CttsError(f"{what}: at most 65535 utterances of 2^24 samples per call, got {B} x {N}")
    _lens_i32(lens, B, what)
    return B, N


def _loudness_tables(edges, chunk_seg, N, what):
    for t, name in ((edges, "edges"), (chunk_seg, "chunk_seg")):
        _p(t)
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise _lib.CttsError(f"{what}: {name} must be a contiguous 1-D int32 device tensor")
    tile = 64 * loudness_chunk()
    if edges.numel() < 2 or chunk_seg.numel() < (N + tile - 1) // tile * 64:
        raise _lib.CttsError(f"{what}: the segment tables do not cover {N} samples")


def kweight_energy(wav, lens, coef, edges, chunk_seg):
    """wav [B,N] float32, lens int32 [B], coef float64 (biquads + state-transition powers), edges / chunk_seg int32 (include/ctts.h) ->
    (hop_sums float64 [B, tiles, slots]: sum of squares of the K-weighted signal per 64-chunk tile and hop segment, zero where a tile
    lies beyond its utterance; peak float32 [B] = max |wav|)"""
    B, N = _loudness_batch(wav, lens, "kweight_energy")
    slots, ncoef, _ = loudness_limits()
    _p(coef)
    if coef.dtype != torch.float64 or not coef.is_contiguous() or coef.numel() != ncoef:
        raise _lib.CttsError(f"kweight_energy: coef must be {ncoef} contiguous float64 words")
    _loudness_tables(edges, chunk_seg, N, "kweight_energy")
    lib = _lib.load()
    dev = wav.device
    tile = 64 * loudness_chunk()
    ws = torch.empty(lib.ctts_loudness_workspace_bytes(B, N) // 8, dtype=torch.float64, device=dev)
    hop_sums = torch.zeros(B, (N + tile - 1) // tile, slots, dtype=torch.float64, device=dev)
    peak = torch.empty(B, dtype=torch.float32, device=dev)
    _lib.check(lib.ctts_kweight_energy(_p(wav), _p(lens), _p(coef), _p(edges), _p(chunk_seg), _p(hop_sums), _p(peak), B, N, edges.numel(),
                                       chunk_seg.numel(), _p(ws), _stream()), "ctts_kweight_energy")
    return hop_sums, peak


def loudness_gate(hop_sums, lens, n_blocks, edges, chunk_seg, blocks, peak, N, block_samples, target=-22.0, peak_limit=True, curve=False):
    """hop_sums / peak of `kweight_energy`, n_blocks int32 [B], blocks int32 [J,2] -> (loudness float64 [B], gain float32 [B],
    valid int32 [B], curve float64 [B,J] or None)"""
    if not torch.is_tensor(hop_sums) or hop_sums.dim() != 3 or hop_sums.dtype != torch.float64 or not hop_sums.is_contiguous():
        raise _lib.CttsError("loudness_gate: expected hop_sums float64 [B, tiles, slots]")
    _p(hop_sums)
    B = hop_sums.shape[0]
    N = int(N)
    slots, _, max_segs = loudness_limits()
    tile = 64 * loudness_chunk()
    if hop_sums.shape[1] != (N + tile - 1) // tile or hop_sums.shape[2] != slots:
        raise _lib.CttsError(f"loudness_gate: hop_sums {tuple(hop_sums.shape)} does not belong to rows of {N} samples")
    _lens_i32(lens, B, "loudness_gate")
    _lens_i32(n_blocks, B, "loudness_gate n_blocks")
    _loudness_tables(edges, chunk_seg, N, "loudness_gate")
    _p(blocks)
    if blocks.dtype != torch.int32 or blocks.dim() != 2 or blocks.shape[1] != 2 or not blocks.is_contiguous() or blocks.shape[0] < 1:
        raise _lib.CttsError("loudness_gate: blocks must be a contiguous int32 [J, 2] device tensor")
    J = blocks.shape[0]
    if J > max_segs or edges.numel() - 2 > max_segs:
        raise _lib.CttsError(f"loudness_gate: at most {max_segs} blocks and hop segments per utterance, got {J} / {edges.numel() - 2}")
    _p(peak)
    if peak.dtype != torch.float32 or peak.numel() != B:
        raise _lib.CttsError("loudness_gate: peak must be float32 [B]")
    dev = hop_sums.device
    loud = torch.empty(B, dtype=torch.float64, device=dev)
    gain = torch.empty(B, dtype=torch.float32, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    cur = torch.empty(B, J, dtype=torch.float64, device=dev) if curve else None
    _lib.check(_lib.load().ctts_loudness_gate(_p(hop_sums), _p(lens), _p(n_blocks), _p(edges), _p(chunk_seg), _p(blocks), _p(peak), _p(loud),
                                              _p(gain), _p(valid), _p(cur), B, N, edges.numel(), chunk_seg.numel(), J, float(block_samples),
                                              float(target), 1 if peak_limit else 0, _stream()), "ctts_loudness_gate")
    return loud, gain, valid, cur


def apply_gain(wav, lens, gain, out=None):
    """out[b][i] = wav[b][i] * gain[b] for i < lens[b], 0 beyond; `out` may be `wav`"""
    B, N = _loudness_batch(wav, lens, "apply_gain")
    _p(gain)
    if gain.dtype != torch.float32 or gain.numel() != B or not gain.is_contiguous():
        raise _lib.CttsError("apply_gain: gain must be float32 [B]")
    if out is None:
        out = torch.empty_like(wav)
    else:
        _p(out)
        if _f32c(out, "out").shape != wav.shape:
            raise _lib.CttsError(f"apply_gain: out {tuple(out.shape)} does not match wav {tuple(wav.shape)}")
    _lib.check(_lib.load().ctts_apply_gain(_p(wav), _p(lens), _p(gain), _p(out), B, N, _stream()), "ctts_apply_gain")
    return out


# ---- waveform metrics: STOI / ESTOI, SI-SDR, multi-resolution STFT distance (csrc/wavmetrics.hip) -----------------------------------
STOI_FRAME, STOI_HOP = 256, 128
MR_STFT_SIZES = (512, 1024, 2048)
WAVMETRICS_MAX_SAMPLES = 1 << 30      # per row (SI-SDR, MR-STFT)


def stoi_max_frames():
    """frames of 256 samples at hop 128 one utterance may hold in `stoi`"""
    return int(_lib.load().ctts_stoi_max_frames())


def _wav_pair(ref, syn, lens, what):
    for t, name in ((ref, "ref"), (syn, "syn")):
        if not torch.is_tensor(t) or t.dim() != 2:
            raise _lib.CttsError(f"{what}: expected {name} [B, N]")
        _p(t)
        _al4(_f32c(t, name), name)
    if ref.shape != syn.shape:
        raise _lib.CttsError(f"{what}: ref {tuple(ref.shape)} and syn {tuple(syn.shape)} must have one shape")
    B, N = ref.shape
    if B < 1 or N < 1:
        raise _lib.CttsError(f"{what}: empty batch {tuple(ref.shape)}")
    if B > 65535 or N > WAVMETRICS_MAX_SAMPLES:
        raise _lib.CttsError(f"{what}: at most 65535 utterances of 2^30 samples per call, got {B} x {N}")
    _lens_i32(lens, B, what)
    return B, N


def _window_f64(window, n, what):
    _p(window)
    if window.dtype != torch.float64 or window.dim() != 1 or window.numel() != n or not window.is_contiguous():
        raise _lib.CttsError(f"{what}: window must be {n} contiguous float64 words on the device")


def stoi(ref, syn, lens, window):
    """ref, syn [B,N] float32 at 10 kHz, lens int32 [B], window float64 [256] -> (stoi float64 [B], estoi float64 [B],
    counts int32 [B,3] = frames, kept frames, segments)"""
    B, N = _wav_pair(ref, syn, lens, "stoi")
    _window_f64(window, STOI_FRAME, "stoi")
    frames = (N - STOI_FRAME) // STOI_HOP + 1 if N >= STOI_FRAME else 0
    if frames > stoi_max_frames():
        raise _lib.CttsError(f"stoi: rows of {N} samples hold {frames} frames; at most {stoi_max_frames()} per utterance")
    lib = _lib.load()
    dev = ref.device
    ws = torch.empty(max(lib.ctts_stoi_workspace_bytes(B, N) // 8, 1), dtype=torch.float64, device=dev)
    d = torch.empty(B, dtype=torch.float64, device=dev)
    e = torch.empty(B, dtype=torch.float64, device=dev)
    counts = torch.empty(B, 3, dtype=torch.int32, device=dev)
    _lib.check(lib.ctts_stoi(_p(ref), _p(syn), _p(lens), _p(window), _p(d), _p(e), _p(counts), B, N, _p(ws), _stream()), "ctts_stoi")
    return d, e, counts


def si_sdr(ref, syn, lens):
    """ref, syn [B,N] float32, lens int32 [B] -> float64 [B] in dB"""
    B, N = _wav_pair(ref, syn, lens, "si_sdr")
    lib = _lib.load()
    ws = torch.empty(max(lib.ctts_si_sdr_workspace_bytes(B, N) // 8, 1), dtype=torch.float64, device=ref.device)
    out = torch.empty(B, dtype=torch.float64, device=ref.device)
    _lib.check(lib.ctts_si_sdr(_p(ref), _p(syn), _p(lens), _p(out), B, N, _p(ws), _stream()), "ctts_si_sdr")
    return out


def mr_stft(ref, syn, lens, window, n_fft, hop):
    """one resolution: ref, syn [B,N] float32, lens int32 [B], window float64 [win] -> (float64 [B,3] = spectral convergence, log-magnitude
    distance, log-spectral distance in dB; frames int32 [B])"""
    B, N = _wav_pair(ref, syn, lens, "mr_stft")
    n_fft, hop = int(n_fft), int(hop)
    if n_fft not in MR_STFT_SIZES:
        raise _lib.CttsError(f"mr_stft: n_fft must be one of {MR_STFT_SIZES}, got {n_fft}")
    if not torch.is_tensor(window) or window.dim() != 1 or not 1 <= window.numel() <= n_fft or hop < 1:
        raise _lib.CttsError(f"mr_stft: need a window of 1 .. n_fft = {n_fft} samples and hop >= 1, got hop {hop}")
    win = window.numel()
    _window_f64(window, win, "mr_stft")
    lib = _lib.load()
    dev = ref.device
    ws = torch.empty(max(lib.ctts_mr_stft_workspace_bytes(B, N, hop, win) // 8, 1), dtype=torch.float64, device=dev)
    out = torch.empty(B, 3, dtype=torch.float64, device=dev)
    frames = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.ctts_mr_stft(_p(ref), _p(syn), _p(lens), _p(window), _p(out), _p(frames), B, N, n_fft, hop, win, _p(ws), _stream()),
               "ctts_mr_stft")
    return out, frames


# ---- speaker embeddings: voice span, filterbank features, NHWC convolution, head (csrc/speaker.hip) ------------------------------------
SPEAKER_NFILT, SPEAKER_BINS = 64, 66
CONV_K5S2_SAME, CONV_K3S1 = 0, 1


def speaker_frames(span):
    """frames of 551 samples at step 221 (the tail zero-padded) of a span of `span` samples; 0 for an empty span"""
    return int(_lib.load().ctts_speaker_frames(int(span)))


def _wav_batch(wav, lens, what):
    if not torch.is_tensor(wav) or wav.dim() != 2:
        raise _lib.CttsError(f"{what}: expected wav [B, N]")
    _p(wav)
    _al4(_f32c(wav, "wav"), "wav")
    B, N = wav.shape
    if B < 1 or N < 1 or B > 65535 or N > 1 << 30:
        raise _lib.CttsError(f"{what}: need 1 .. 65535 utterances of 1 .. 2^30 samples, got {tuple(wav.shape)}")
    if lens is not None:
        _lens_i32(lens, B, what)
    return B, N


def _i32_vec(t, n, name, what):
    _p(t)
    if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise _lib.CttsError(f"{what}: {name} must be {n} contiguous int32 words on the device")
    return t


def speaker_span(wav, lens):
    """wav [B,N] float32, lens int32 [B] -> (first, last, n_frames, valid) int32 [B]: the span x[first:last] above the 95th percentile of
    |x|, its fbank frame count and whether it holds a sample"""
    B, N = _wav_batch(wav, lens, "speaker_span")
    first, last, frames, valid = (torch.empty(B, dtype=torch.int32, device=wav.device) for _ in range(4))
    _lib.check(_lib.load().ctts_speaker_span(_p(wav), _p(lens), _p(first), _p(last), _p(frames), _p(valid), B, N, _stream()),
               "ctts_speaker_span")
    return first, last, frames, valid


def speaker_fbank(wav, first, last, valid, bins, out_frames, offsets=None, centre=False):
    """wav [B,N] float32 and the span of `speaker_span`, bins int32 [66] -> normalised filterbank features float32 [B, out_frames, 64];
    row j is frame r + j with r = offsets[b], else the centre crop when `centre`, else 0"""
    B, N = _wav_batch(wav, None, "speaker_fbank")
    for t, name in ((first, "first"), (last, "last"), (valid, "valid")):
        _i32_vec(t, B, name, "speaker_fbank")
    _i32_vec(bins, SPEAKER_BINS, "bins", "speaker_fbank")
    if offsets is not None:
        _i32_vec(offsets, B, "offsets", "speaker_fbank")
    out_frames = int(out_frames)
    if out_frames < 1:
        raise _lib.CttsError(f"speaker_fbank: out_frames must be >= 1, got {out_frames}")
    out = torch.empty(B, out_frames, SPEAKER_NFILT, dtype=torch.float32, device=wav.device)
    _lib.check(_lib.load().ctts_speaker_fbank(_p(wav), _p(first), _p(last), _p(valid), _p(bins), _p(offsets), _p(out), B, N, out_frames,
                                              1 if centre else 0, _stream()), "ctts_speaker_fbank")
    return out


def conv2d_nhwc_out_hw(H, W, geom):
    s = 2 if geom == CONV_K5S2_SAME else 1
    return -(-H // s), -(-W // s)


def conv2d_nhwc(x, w, bias, geom, lo, hi, res=None, out=None):
    """x [B,H,W,Cin] float32 NHWC, w [k,k,Cin,Cout], bias [Cout] -> clip(conv + bias) [B,Ho,Wo,Cout], or clip(clip(conv + bias) + res)
    with a residual shaped like the output; geom CONV_K5S2_SAME (5 x 5, stride 2, TF 'same') or CONV_K3S1 (3 x 3, stride 1, pad 1)"""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise _lib.CttsError("conv2d_nhwc: expected x [B, H, W, Cin]")
    for t, name in ((x, "x"), (w, "w"), (bias, "bias")):
        _p(t)
        _f32c(t, name)
    if geom not in (CONV_K5S2_SAME, CONV_K3S1):
        raise _lib.CttsError(f"conv2d_nhwc: unknown geometry {geom}")
    B, H, W, Cin = x.shape
    k = 5 if geom == CONV_K5S2_SAME else 3
    if w.dim() != 4 or tuple(w.shape[:3]) != (k, k, Cin):
        raise _lib.CttsError(f"conv2d_nhwc: w {tuple(w.shape)} is not [{k}, {k}, {Cin}, Cout]")
    Cout = w.shape[3]
    if tuple(bias.shape) != (Cout,):
        raise _lib.CttsError(f"conv2d_nhwc: bias {tuple(bias.shape)} is not [{Cout}]")
    Ho, Wo = conv2d_nhwc_out_hw(H, W, geom)
    shape = (B, Ho, Wo, Cout)
    if res is not None:
        _p(res)
        if tuple(_f32c(res, "res").shape) != shape:
            raise _lib.CttsError(f"conv2d_nhwc: res {tuple(res.shape)} does not match the output {shape}")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        _p(out)
        if tuple(_f32c(out, "out").shape) != shape:
            raise _lib.CttsError(f"conv2d_nhwc: out {tuple(out.shape)} does not match {shape}")
    lib = _lib.load()
    nbytes = lib.ctts_conv2d_nhwc_workspace_bytes(B, H, W, Cin, Cout, geom)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device) if nbytes else None
    _lib.check(lib.ctts_conv2d_nhwc(_p(x), _p(w), _p(bias), _p(res), _p(out), B, H, W, Cin, Cout, geom, 0 if res is None else 1,
                                    float(lo), float(hi), _p(ws), _stream()), "ctts_conv2d_nhwc")
    return out


def speaker_head(x, w, bias, valid=None):
    """x [B,T,F] float32, w [F,E], bias [E] -> the L2-normalised affine image of the time mean, float32 [B,E]; zeros where valid == 0"""
    if not torch.is_tensor(x) or x.dim() != 3:
        raise _lib.CttsError("speaker_head: expected x [B, T, F]")
    for t, name in ((x, "x"), (w, "w"), (bias, "bias")):
        _p(t)
        _f32c(t, name)
    B, T, F = x.shape
    if w.dim() != 2 or w.shape[0] != F or tuple(bias.shape) != (w.shape[1],):
        raise _lib.CttsError(f"speaker_head: w {tuple(w.shape)} / bias {tuple(bias.shape)} do not fit x {tuple(x.shape)}")
    E = w.shape[1]
    if valid is not None:
        _i32_vec(valid, B, "valid", "speaker_head")
    out = torch.empty(B, E, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().ctts_speaker_head(_p(x), _p(w), _p(bias), _p(valid), _p(out), B, T, F, E, _stream()), "ctts_speaker_head")
    return out
