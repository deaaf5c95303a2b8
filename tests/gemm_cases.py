"""The case table of the GEMM contract tests: one list, read by tests/test_gemm_restate_cpu.py (route kinds and completeness, no GPU) and by
tests/test_gemm_contract_gpu.py (every case launched and compared with tests/gemm_restate64.py).

A case is (id, kind it must route to, layout, (M, N, K), feature, recipe); `build` turns it into host buffers with guard cells and the
keyword arguments of kernels._gemm_desc, `route_of` asks ctts_gemm_route for it (host code: no pointer is dereferenced, so the operands
may be CPU tensors) and `bound_of` gives the bound of a random-recipe case.

Kinds covered: scalar64, buf64, buf_k2, buf_narrow, x6, x6tn, weight_stationary, planes, planes_wgrad, stream_k.
Kinds left to their existing tests:
  - vec64 / vec128 need an operand beyond 2 GiB: tests/test_kernels_gpu.py::test_pointer_vec_route_kinds_run_an_operand_beyond_the_buffer_window;
  - buf128 needs CTTS_FORCE_TILE, an environment knob read once per process: tests/test_gemm_route_cpu.py names it, no launch test;
  - bf16_split 3 and 4 are reduced precision: tests/test_amp_gpu.py.

Shapes (SHAPES): per kind the smallest shape of tests/test_gemm_route_cpu.py, then M and N one below, on and one above a multiple of the
kind's tile and K one granule up and off the granule - where ctts_gemm_route, asked on this machine, still names the kind.
Features (FEATURES): each switched on at the kind's EDGE shape; TAKES lists the (kind, feature) pairs for which the route stays with the
kind - the CPU test asserts that list against the route query at the kind's BASE shape, pair by pair, in both directions.

Two operand recipes.  exact: 18-bit integers against sparse +-1 (test_kernels_gpu._route_exact, with the density raised for short K so
that no output column is all zero: every column of the +-1 operand keeps fewer than 128 non-zeros, so every partial sum stays below
2^24), alpha a power of two, small-integer bias / R / Z, rowscale in {0, 1}, activation none or relu, dropout with p = 0.5 (scale 2):
every fp32 partial sum is an exact integer on every family, the comparison is equality.  random: the operands of the family's own
test, the family's own bound (bound_of)."""
import collections
import contextlib
import zlib

import numpy as np
import torch

from ctts_amd import kernels as K

Case = collections.namedtuple("Case", "id kind layout M N K feature recipe")

KINDS = ("scalar64", "buf64", "buf_k2", "buf_narrow", "x6", "x6tn", "weight_stationary", "planes", "planes_wgrad", "stream_k")
TILE = {"scalar64": (64, 64), "buf64": (64, 64), "buf_k2": (32, 64), "buf_narrow": (128, 32), "x6": (128, 128), "x6tn": (128, 128),
        "weight_stationary": (64, 128), "planes": (128, 256), "planes_wgrad": (128, 256), "stream_k": (128, 128)}
GRANULE = {k: 64 if k == "buf_k2" else 32 for k in KINDS}
SK_RAGGED_TILE = (64, 256)      # stream_k with a tile_map: the m-tile schedule is built for 64-row tiles, the tile is 256 columns wide instead
# what every descriptor of a kind carries (the route's size thresholds off, the persistent kernel asked for only where it is the subject)
FIXED = {"scalar64": dict(bf16_split=0, use_sk=False), "buf64": dict(bf16_split=0, use_sk=False), "buf_k2": dict(bf16_split=0, use_sk=False),
         "buf_narrow": dict(bf16_split=0, use_sk=False), "x6": dict(bf16_split=2, use_sk=False), "x6tn": dict(bf16_split=2, use_sk=False, split_k=2),
         "weight_stationary": dict(bf16_split=0, use_sk=False), "planes": dict(bf16_split=2, planes=True),
         "planes_wgrad": dict(bf16_split=2, planes=True, split_k=2), "stream_k": dict(bf16_split=0, use_sk=True)}
# (layout, M, N, K): the smallest shape a kind takes (tests/test_gemm_route_cpu.py ROWS; stream_k: the smallest ctts_gemm_sk_plan accepts)
BASE = {"scalar64": ("NT", 70, 50, 30), "buf64": ("NT", 130, 130, 64), "buf_k2": ("NT", 256, 64, 256), "buf_narrow": ("NT", 256, 32, 64),
        "x6": ("NT", 1024, 128, 256), "x6tn": ("TN", 128, 128, 2048), "weight_stationary": ("NT", 4096, 64, 256),
        "planes": ("NT", 128, 256, 64), "planes_wgrad": ("TN", 128, 256, 64), "stream_k": ("NT", 2048, 2048, 2048)}
# the edge shape the features are switched on at: M, N, K beside a tile / granule edge where the kind allows it
EDGE = {"scalar64": ("NT", 71, 65, 30), "buf64": ("NT", 129, 131, 68), "buf_k2": ("NT", 257, 65, 260), "buf_narrow": ("NT", 257, 31, 68),
        "x6": ("NT", 1025, 128, 288), "x6tn": ("TN", 128, 128, 2080), "weight_stationary": ("NT", 4097, 129, 256),
        "planes": ("NT", 129, 256, 96), "planes_wgrad": ("TN", 128, 256, 100), "stream_k": ("NT", 2049, 2048, 2080)}
# conv views: (conv_T, channels for 3 taps, channels for 9 taps); conv_T is no multiple of a tile, so tiles straddle utterance boundaries
CONV_A = {"scalar64": (37, 4, 4), "buf64": (37, 8, 8), "buf_k2": (37, 88, 32), "buf_narrow": (37, 24, 8), "x6": (37, 96, 32),
          "weight_stationary": (37, 84, 28), "planes": (37, 32, 32), "stream_k": (150, 704, 256), "x6tn": (40, 128, 128),
          "planes_wgrad": (40, 256, 256)}
CONV_B = {"scalar64": (37, 4, 4), "buf64": (37, 8, 8), "buf_k2": (37, 24, 8), "buf_narrow": (37, 4, 4), "x6": (40, 128, 128),
          "weight_stationary": (37, 24, 8), "planes": (40, 256, 256), "stream_k": (150, 704, 256), "x6tn": (40, 128, 128),
          "planes_wgrad": (40, 256, 256)}
# padded-row features: rows per utterance where the generic 2 * tile_m + 6 does not suit the kind, as (M or reduction rows, row_T)
ROWS = {"planes": (512, 256), "planes_wgrad": (128, 64), "x6tn": (2080, 104)}

FORWARD = ("epi_act0", "epi_act1", "epi_act2", "epi_act3", "epi_act4", "epi_res", "epi_drop", "epi_drop_act2", "epi_full")
BACKWARD = tuple(f"bwd_act{a}{d}" for a in range(5) for d in ("", "_drop"))
FEATURES = ("offsets", "lim_m", "lim_n", "lim_k", "conv3", "conv9", "tn_conv3", "tn_conv9",
            "split2_add", "split3_add", "split2_ow", "split3_ow", "split2_defer", "split3_defer") + FORWARD + \
           ("rows_h0", "rows_h0_map", "rows_h4", "rows_h4_map", "softmax_bwd") + BACKWARD + ("c_planes",)
RANDOM = {"epi_act2", "epi_act3", "epi_act4", "epi_drop_act2", "epi_full", "softmax_bwd", "bwd_act2", "bwd_act3", "bwd_act4", "bwd_act2_drop",
          "bwd_act3_drop", "bwd_act4_drop"}


def _fake_ws():
    from ctts_amd import _lib
    n = _lib.load().ctts_workspace_bytes()
    return collections.namedtuple("FakeWs", "data_ptr numel")(lambda: 0x7E0000000000, lambda: n)


@contextlib.contextmanager
def host_pointers():
    """kernels._gemm_desc on CPU tensors, for queries that dereference nothing: every storage gets a made-up, 4 KiB-aligned address 64 GiB
    from the next one (the alignment of an operand inside its storage is kept), the workspace a made-up one of the right size"""
    slots = {}

    def p(t, offset=0):
        if t is None:
            return None
        key = t.untyped_storage().data_ptr()
        slot = slots.setdefault(key, len(slots) + 1)
        return 0x7F0000000000 + slot * (1 << 36) + (t.storage_offset() + offset) * t.element_size()

    saved = K._p, K.gemm_workspace
    ws = _fake_ws()
    K._p, K.gemm_workspace = p, lambda device: ws
    try:
        yield
    finally:
        K._p, K.gemm_workspace = saved


def _rng(case_id):
    return torch.Generator().manual_seed(zlib.crc32(case_id.encode()))


def _sentinel(n, salt):
    """finite, integer-valued, different from cell to cell"""
    i = np.arange(n, dtype=np.int64)
    return torch.from_numpy((((i * 7919 + salt * 104729) % 2039) - 1019).astype(np.float32))


def _small_ints(shape, g, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


class Problem:
    """host buffers (flat float32, guards included) + the arguments of kernels.gemm / gemm_restate64.restate"""

    def __init__(self):
        self.kw = {}            # keyword arguments with HOST tensors
        self.planes = self.want_map = self.defer = self.want_c_planes = False


def build(case, contents=True):
    """contents=False: the operands are left zero (route queries look at addresses and sizes only)"""
    kind, layout, M, N, K_, feat = case.kind, case.layout, case.M, case.N, case.K, case.feature
    g = _rng(case.id)
    exact = case.recipe == "exact"
    tile_m, tile_n = TILE[kind]
    fixed = dict(FIXED[kind])
    p = Problem()
    p.case = case
    p.planes = bool(fixed.pop("planes", False))
    kw = p.kw
    kw.update(fixed)
    unaligned = kind == "scalar64"
    al = 32 if p.planes else 4                      # leading dimensions / offsets keep this alignment (scalar64: none)
    conv = None
    if feat in ("conv3", "conv9"):
        layout = "NT"
        T, c3, c9 = CONV_A[kind]
        cin, taps = (c3, 3) if feat == "conv3" else (c9, 9)
        K_ = cin * taps
        M = -(-M // T) * T                          # whole utterances: the view tests t against conv_T only
        conv = (T, taps // 2, cin)
    elif feat in ("tn_conv3", "tn_conv9"):
        layout = "TN"
        T, c3, c9 = CONV_B[kind]
        cin, taps = (c3, 3) if feat == "tn_conv3" else (c9, 9)
        N = cin * taps
        K_ = -(-K_ // T) * T
        conv = (T, taps // 2, cin)
        kw["conv_on_b"] = True
    if feat in FORWARD or feat in BACKWARD or feat in ("softmax_bwd", "c_planes"):
        kw.pop("split_k", None)                     # an epilogue excludes split-K: the kinds whose base carries split_k = 2 drop it here
    rows = feat.startswith("rows_")
    a_kc, b_kc = {"NT": (True, True), "NN": (True, False), "TN": (False, False)}[layout]
    if rows and kind in ROWS:
        if a_kc:
            M = ROWS[kind][0]
        else:
            K_ = ROWS[kind][0]
    if feat.endswith("_defer"):
        N = -(-N // 4) * 4                          # ctts_partial_sums adds dense [M, N] matrices: N a multiple of 4
    if feat == "c_planes":
        N = -(-N // 32) * 32
    p.layout, p.M, p.N, p.K = layout, M, N, K_
    # ---- geometry of A, B
    a_rows, a_cols = (M, K_) if a_kc else (K_, M)
    b_rows, b_cols = (N, K_) if b_kc else (K_, N)
    pad_ld = feat == "offsets"
    lda = a_cols + (0 if (conv and not kw.get("conv_on_b")) or not pad_ld else (al if not unaligned else 3))
    ldb = b_cols + (0 if (conv and kw.get("conv_on_b")) or not pad_ld else (al if not unaligned else 5))
    if p.planes:
        lda, ldb = -(-lda // 32) * 32, -(-ldb // 32) * 32
    if conv:                                        # a conv operand is dense with ld = conv_cin; its rows are the (b, t) rows
        if kw.get("conv_on_b"):
            ldb, b_rows, b_cols = conv[2], K_, conv[2]
        else:
            lda, a_rows, a_cols = conv[2], M, conv[2]
    a_off = b_off = 0
    if pad_ld:
        a_off, b_off = (2 * lda, 3 * ldb) if not unaligned else (2 * lda + 1, 3 * ldb + 2)
        if not p.planes and not unaligned:
            a_off, b_off = a_off + 4, b_off + 8
    if unaligned and (K_ % 4 == 0 if (a_kc and b_kc) else False):
        b_off += 1                                  # keep the launch off the 16-byte loaders: an operand base that is not 16-byte aligned
    batched = feat in ("lim_m", "lim_n", "lim_k")
    nb0, nb1 = (3, 2) if batched else (1, 1)
    a_blk, b_blk = a_rows * lda, b_rows * ldb
    sA = (2 * (a_blk + 8) + 12, a_blk + 8) if batched else (0, 0)
    sB = (2 * (b_blk + 4) + 16, b_blk + 4) if batched else (0, 0)
    conv_halo = (conv[1] * conv[2] + 3) // 4 * 4 if conv else 0      # room the conv view's shifted rows may be ADDRESSED in (never read)
    if conv and not kw.get("conv_on_b"):
        a_off += conv_halo
    if conv and kw.get("conv_on_b"):
        b_off += conv_halo
    a_len = a_off + (nb0 - 1) * sA[0] + (nb1 - 1) * sA[1] + a_blk + conv_halo + 64
    b_len = b_off + (nb0 - 1) * sB[0] + (nb1 - 1) * sB[1] + b_blk + conv_halo + 64
    # ---- operands
    if not contents:
        A, Bm = torch.zeros(a_len), torch.zeros(b_len)
    elif exact:
        A = torch.randint(-(1 << 17), (1 << 17) + 1, (a_len,), generator=g).float()
        dens = min(0.5, 48.0 / max(K_, 1))
        Bm = (torch.randint(0, 2, (b_len,), generator=g) * 2 - 1).float() * (torch.rand(b_len, generator=g) < dens)
    elif kind == "weight_stationary":
        A, Bm = torch.randn(a_len, generator=g), torch.randn(b_len, generator=g) * 0.05
    elif kind == "stream_k":
        A, Bm = torch.rand(a_len, generator=g) - 0.5, (torch.rand(b_len, generator=g) - 0.5) * 0.1
    elif kind in ("planes", "planes_wgrad"):
        A, Bm = torch.rand(a_len, generator=g) * 2 - 1, torch.rand(b_len, generator=g) * 2 - 1
    else:
        A, Bm = torch.rand(a_len, generator=g) * 2 - 1, (torch.rand(b_len, generator=g) * 2 - 1) * 0.3
    # ---- C with guards: a tile of rows in front, one behind, ldc > N
    padc = 3 if unaligned else (32 if kind in ("weight_stationary", "planes", "planes_wgrad", "stream_k", "x6", "x6tn") else 4)
    ldc = N + padc
    c_off = tile_m * ldc + (padc // 2 if pad_ld else 0)
    sC = (2 * ((M + 2) * ldc + 4) + 5 * ldc, (M + 2) * ldc + 4) if batched else (0, 0)
    c_len = c_off + (nb0 - 1) * sC[0] + (nb1 - 1) * sC[1] + (M + tile_m) * ldc
    Cb = _sentinel(c_len, 1)
    p.A, p.B, p.C = A, Bm, Cb
    p.lda, p.ldb, p.ldc, p.a_kc, p.b_kc = lda, ldb, ldc, a_kc, b_kc
    kw.update(a_off=a_off, b_off=b_off, c_off=c_off)
    if batched:
        kw.update(nb0=nb0, nb1=nb1, sA=sA, sB=sB, sC=sC)
        i = ("lim_m", "lim_n", "lim_k").index(feat)
        full = (M, N, K_)[i]
        kw.update(lens=torch.tensor([1, full, full // 2 + 1], dtype=torch.int32), lim=tuple(int(j == i) for j in range(3)))
    if conv:
        kw["conv"] = conv
    alpha_exact = 0.5
    # ---- split-K
    if feat.startswith("split"):
        kw["split_k"] = int(feat[5])
        kw["split_overwrite"] = feat.endswith("_ow")
        p.defer = feat.endswith("_defer")
        kw["alpha"] = alpha_exact
    if kw.get("split_k", 1) > 1 and "alpha" not in kw:
        kw["alpha"] = alpha_exact

    def guarded(ld, salt, values=None):
        """[tile_m + M + tile_m, ld] flat, sentinels, optionally `values` [M, N] in the block; -> (full buffer, view the descriptor gets)"""
        full = _sentinel((2 * tile_m + M) * ld, salt)
        if values is not None:
            full.view(-1, ld)[tile_m:tile_m + M, :N] = values
        return full, full[tile_m * ld:]

    ldx = N + padc
    fwd = feat in FORWARD
    if fwd:
        a = {"epi_act0": 0, "epi_act1": 1, "epi_act2": 2, "epi_act3": 3, "epi_act4": 4, "epi_res": 0, "epi_drop": 0, "epi_drop_act2": 2,
             "epi_full": 2}[feat]
        kw["act"] = a
        kw["alpha"] = alpha_exact if exact else 0.7
        kw["bias"] = _small_ints((N,), g) * 1024 if exact else torch.rand(N, generator=g) * 2 - 1
        if a or feat == "epi_full":
            p.Zfull, kw["Z"] = guarded(ldx, 2)
            kw["ldz"] = ldx
        if feat in ("epi_res", "epi_drop", "epi_full"):
            vals = _small_ints((M, N), g) if exact else torch.randn(M, N, generator=g)
            p.Rfull, kw["R"] = guarded(ldx, 3, vals)
            kw["ldr"] = ldx
            kw["rowscale"] = (torch.rand(M, generator=g) > 0.3).float()
        if feat in ("epi_drop", "epi_drop_act2", "epi_full"):
            kw.update(p_drop=0.5 if exact else 0.25, seed=torch.tensor([0x5DEECE66D1234567 + M], dtype=torch.int64), drop_offset=11)
    if feat in BACKWARD:
        a = int(feat[7])
        kw.update(epi_bwd=True, act=a, alpha=alpha_exact if exact else 0.7)
        if a:
            vals = _small_ints((M, N), g) if exact else torch.randn(M, N, generator=g)
            p.Zfull, kw["Z"] = guarded(ldx, 2, vals)
            kw["ldz"] = ldx
        if feat.endswith("_drop"):
            kw.update(p_drop=0.5 if exact else 0.25, seed=torch.tensor([0x1234567 + N], dtype=torch.int64), drop_offset=7)
    if feat == "c_planes":
        kw.update(epi_bwd=True, alpha=alpha_exact)
        p.want_c_planes = True
    if feat == "softmax_bwd":
        e_len = c_len - c_off
        kw.update(E=torch.rand(e_len, generator=g), rowsub=torch.rand(nb0 * nb1 * M, generator=g) - 0.5, alpha=0.7)
    if rows:
        halo = 4 if "_h4" in feat else 0
        n_rows = M if a_kc else K_
        T = ROWS[kind][1] if kind in ROWS else min(n_rows, 2 * tile_m + 6)
        nutt = -(-n_rows // T)
        lens = [3, T, T // 2 + 1, 1, T - 1, 2 * T // 3]
        lens = (lens * (nutt // len(lens) + 1))[:nutt]
        kw.update(row_lens=torch.tensor(lens, dtype=torch.int32), row_T=T, row_halo=halo)
        p.want_map = feat.endswith("_map")
        # the caller's duty (include/ctts.h): rows of A beyond an utterance's length + halo are zero
        r = torch.arange(n_rows)
        dead = r % T >= torch.tensor(lens)[r // T] + halo
        view = A[a_off:a_off + n_rows * lda].view(n_rows, lda)
        view[dead] = 0.0
        if "alpha" not in kw:
            kw["alpha"] = alpha_exact
    return p


def restate_args(p):
    """(positional, keyword) arguments of gemm_restate64.restate for a built problem (host tensors)"""
    kw = {k: v for k, v in p.kw.items() if k not in ("bf16_split", "use_sk")}
    return (p.A, p.B, p.C, p.M, p.N, p.K, p.lda, p.ldb, p.ldc, p.a_kc, p.b_kc), kw


def device_args(p, dev):
    """(positional, keyword) arguments of kernels.gemm / gemm_route on `dev`, and the device tensors by name.  On the CPU (inside
    host_pointers()) the plane sets and the tile map are stand-ins: the route only looks at their addresses."""
    on_gpu = torch.device(dev).type != "cpu"
    t = {}

    def to(x):
        return x.to(dev) if on_gpu else x

    t["A"], t["B"], t["C"] = to(p.A), to(p.B), to(p.C.clone())
    kw = {}
    for k, v in p.kw.items():
        if k in ("Z", "R"):
            full = to(getattr(p, k + "full").clone())
            t[k + "full"] = full
            off = full.numel() - v.numel()
            kw[k] = full[off:]
        elif torch.is_tensor(v):
            t[k] = kw[k] = to(v)
        else:
            kw[k] = v
    if p.planes:
        a_off, b_off = p.kw["a_off"], p.kw["b_off"]
        assert a_off % p.lda == 0 and b_off % p.ldb == 0
        ma, mb = t["A"][:t["A"].numel() // p.lda * p.lda].view(-1, p.lda), t["B"][:t["B"].numel() // p.ldb * p.ldb].view(-1, p.ldb)
        if on_gpu:
            pa, pb = K.split_planes([ma, mb])
        else:
            pa, pb = (torch.zeros(m.shape[0], p.lda // 32, 3, 32, dtype=torch.bfloat16) for m in (ma, mb))
        t["a_planes"], t["b_planes"] = pa, pb
        kw["a_planes"], kw["b_planes"] = pa[a_off // p.lda:], pb[b_off // p.ldb:]
    if p.want_map:
        tm_rows = p.M
        kw["tile_map"] = K.row_tile_map(kw["row_lens"], p.kw["row_T"], p.kw["row_halo"], tm_rows) if on_gpu else \
            torch.zeros(1 + (tm_rows + 63) // 64, dtype=torch.int32)
    if p.want_c_planes:
        rows_total = t["C"].numel() // p.ldc
        cp = torch.full((rows_total, p.ldc // 32, 3, 32), 0x1234, dtype=torch.int16).view(torch.bfloat16)
        t["c_planes_full"] = to(cp)
        assert p.kw["c_off"] % p.ldc == 0
        kw["c_planes"] = t["c_planes_full"][p.kw["c_off"] // p.ldc:]
    args = (t["A"], t["B"], t["C"], p.M, p.N, p.K, p.lda, p.ldb, p.ldc, p.a_kc, p.b_kc)
    return args, kw, t


def route_of(p):
    """GemmRoute of a built problem, asked with host pointers"""
    with host_pointers():
        args, kw, _ = device_args(p, "cpu")
        return K.gemm_route(*args, **kw)


def split_plan_of(args, kw):
    """(count, stride) when ctts_gemm_split_plan lets the caller keep the partial matrices of this launch, else None"""
    import ctypes as C
    from ctts_amd import _lib
    d, cnt, stride = K._gemm_desc(*args, **kw), C.c_int32(0), C.c_int64(0)
    if _lib.load().ctts_gemm_split_plan(C.byref(d), C.byref(cnt), C.byref(stride)) != 1:
        return None
    return cnt.value, stride.value


def takes(p, kind):
    """the route of the built problem is `kind` - and, for a deferred split, the split plan lets the caller keep the partials (a kind
    that finishes its sum itself does not take a descriptor with split_out)"""
    with host_pointers():
        args, kw, _ = device_args(p, "cpu")
        if K.gemm_route(*args, **kw).kind != kind:
            return False
        return not p.defer or split_plan_of(args, kw) is not None


def product_bound(kind, Kd):
    """bound on max |C - float64| given max |float64| of a plain product, per family: tests/test_kernels_gpu.py _ROUTE_CASES"""
    if kind in ("scalar64", "buf64", "buf_k2", "buf_narrow"):
        return lambda s: 2e-6 * max(1, Kd / 16) * max(1.0, s)              # test_gemm_nt
    if kind in ("weight_stationary", "planes"):
        return lambda s: 2e-5 * max(1.0, s)                                # test_weight_stationary_gemm_..., test_planes_gpu ..._vs_fp64
    if kind == "planes_wgrad":
        return lambda s: 2e-6 * s                                          # test_planes_wgrad_gpu close()
    if kind == "stream_k":
        return lambda s: 2e-5                                              # test_dominant_stream_k_kernel_vs_fp64_... (its operands)
    return None                                                            # x6 / x6tn: exact cases only, or against the fp32 kernels


def bound_of(case):
    """(bound of C, bound of Z), each a function of max |float64|, for a random-recipe case.  The epilogue cases take the bounds of
    test_gemm_lean_epilogue_modes_vs_fp64 / test_gemm_epilogue_all (tile kernels and weight-stationary: C 2e-5, Z 1e-5, times
    max(1, |ref|max)) and of the plane and stream-K tests (2e-5 times max(1, |ref|max), resp. 2e-5 absolute on their operands);
    softmax_bwd has no epilogue rounding beyond the product's two operations and keeps the family's product bound.
    x6 / x6tn have no float64 bound of their own for an epilogue term: (None, None) tells the GPU test to measure the error of the
    fp32-MFMA kernels on the same descriptor and bound the case by it (x6: twice that; x6tn: its own test's 2.5 * e32 + 1e-6)."""
    kind = case.kind
    if kind in ("x6", "x6tn"):
        return None, None
    if case.feature == "softmax_bwd":
        return product_bound(kind, case.K), None
    if kind == "stream_k":
        return (lambda s: 2e-5), (lambda s: 2e-5)
    if kind in ("planes", "planes_wgrad"):
        return (lambda s: 2e-5 * max(1.0, s)), (lambda s: 2e-5 * max(1.0, s))
    return (lambda s: 2e-5 * max(1.0, s)), (lambda s: 1e-5 * max(1.0, s))


# ---- the table ---------------------------------------------------------------------------------------------------------------------
# shape-edge cases: (layout, M, N, K) per kind, all with the exact recipe
SHAPES = {
    "scalar64": [("NT", 70, 50, 30), ("NT", 63, 64, 30), ("NT", 64, 65, 31), ("NT", 65, 63, 33), ("NT", 127, 129, 62), ("NT", 128, 128, 65),
                 ("NT", 129, 127, 1), ("NN", 65, 63, 33), ("NN", 128, 129, 64), ("TN", 63, 65, 64), ("TN", 129, 66, 33), ("NT", 1, 1, 7)],
    "buf64": [("NT", 130, 130, 64), ("NT", 63, 64, 64), ("NT", 64, 65, 96), ("NT", 65, 63, 68), ("NT", 127, 128, 36), ("NT", 128, 129, 100),
              ("NT", 129, 127, 4), ("NN", 129, 132, 68), ("NN", 64, 124, 96), ("TN", 132, 124, 65), ("TN", 64, 68, 33), ("NT", 1, 1, 4)],
    "buf_k2": [("NT", 256, 64, 256), ("NT", 257, 65, 260), ("NT", 287, 127, 320), ("NT", 288, 128, 256), ("NT", 289, 129, 324),
               ("NT", 256, 191, 316), ("NN", 257, 68, 260), ("NN", 288, 128, 320), ("TN", 260, 64, 257), ("TN", 288, 132, 321)],
    "buf_narrow": [("NT", 256, 32, 64), ("NT", 257, 31, 68), ("NT", 383, 32, 96), ("NT", 384, 1, 36), ("NT", 385, 17, 100),
                   ("NN", 257, 28, 68), ("NN", 384, 32, 36), ("TN", 260, 32, 65), ("TN", 384, 4, 64)],
    "x6": [("NT", 1024, 128, 256), ("NT", 1025, 128, 288), ("NT", 1151, 256, 256), ("NT", 1152, 128, 320), ("NT", 1153, 384, 256)],
    "x6tn": [("TN", 128, 128, 2048), ("TN", 128, 128, 2080), ("TN", 256, 128, 2048), ("TN", 128, 256, 2112)],
    "weight_stationary": [("NT", 4096, 64, 256), ("NT", 4097, 129, 256), ("NT", 4159, 127, 256), ("NT", 4160, 128, 256), ("NT", 4161, 65, 256),
                          ("NT", 4100, 255, 256), ("NN", 4097, 132, 256), ("NN", 4160, 64, 256)],
    "planes": [("NT", 128, 256, 64), ("NT", 129, 256, 96), ("NT", 255, 384, 64), ("NT", 256, 512, 128), ("NT", 257, 256, 64)],
    "planes_wgrad": [("TN", 128, 256, 64), ("TN", 128, 256, 100), ("TN", 256, 256, 65), ("TN", 128, 512, 96), ("TN", 128, 256, 127)],
    # 2048^3: the smallest launch ctts_gemm_sk_plan accepts (256 tiles of 128 x 128 for the 512-workgroup grid; 1920 rows are refused);
    # 2049 rows: 272 tiles x 65 K-blocks, which do not divide evenly over the grid
    "stream_k": [("NT", 2048, 2048, 2048), ("NT", 2049, 2048, 2080), ("NN", 2047, 2052, 2048), ("TN", 2052, 2044, 2112)],
}
# (kind, feature) pairs whose route stays with the kind
TAKES = {
    "scalar64": ("offsets", "lim_m", "lim_n", "lim_k", "conv3", "conv9", "tn_conv3", "tn_conv9", "split2_add", "split3_add", "split2_ow", "split3_ow",
        "split2_defer", "split3_defer", "epi_act0", "epi_act1", "epi_act2", "epi_act3", "epi_act4", "epi_res", "epi_drop", "epi_drop_act2",
        "epi_full", "rows_h0", "rows_h0_map", "rows_h4", "rows_h4_map", "softmax_bwd", "bwd_act0", "bwd_act0_drop", "bwd_act1", "bwd_act1_drop",
        "bwd_act2", "bwd_act2_drop", "bwd_act3", "bwd_act3_drop", "bwd_act4", "bwd_act4_drop", "c_planes"),
    "buf64": ("offsets", "lim_m", "lim_n", "lim_k", "conv3", "conv9", "split2_add", "split3_add", "split2_ow", "split3_ow", "split2_defer",
        "split3_defer", "epi_act0", "epi_act1", "epi_act2", "epi_act3", "epi_act4", "epi_res", "epi_drop", "epi_drop_act2", "epi_full", "rows_h0",
        "rows_h0_map", "rows_h4", "rows_h4_map", "softmax_bwd", "bwd_act0", "bwd_act0_drop", "bwd_act1", "bwd_act1_drop", "bwd_act2", "bwd_act2_drop",
        "bwd_act3", "bwd_act3_drop", "bwd_act4", "bwd_act4_drop", "c_planes"),
    "buf_k2": ("offsets", "conv3", "conv9", "tn_conv3", "tn_conv9", "split2_add", "split3_add", "split2_ow", "split3_ow", "split2_defer",
        "split3_defer", "epi_act0", "epi_act1", "epi_act2", "epi_act3", "epi_act4", "epi_res", "epi_drop", "epi_drop_act2", "epi_full", "rows_h0",
        "rows_h0_map", "rows_h4", "rows_h4_map", "softmax_bwd", "bwd_act0", "bwd_act0_drop", "bwd_act1", "bwd_act1_drop", "bwd_act2", "bwd_act2_drop",
        "bwd_act3", "bwd_act3_drop", "bwd_act4", "bwd_act4_drop", "c_planes"),
    "buf_narrow": ("offsets", "lim_m", "lim_n", "lim_k", "split2_add", "split3_add", "split2_ow", "split3_ow", "split2_defer", "split3_defer",
        "epi_act0", "epi_act1", "epi_act2", "epi_act3", "epi_act4", "epi_res", "epi_drop", "epi_drop_act2", "epi_full", "softmax_bwd", "bwd_act0",
        "bwd_act0_drop", "bwd_act1", "bwd_act1_drop", "bwd_act2", "bwd_act2_drop", "bwd_act3", "bwd_act3_drop", "bwd_act4", "bwd_act4_drop",
        "c_planes"),
    "x6": ("offsets", "conv3", "conv9", "epi_act0", "epi_act1", "epi_act2", "epi_act3", "epi_act4", "epi_res", "epi_drop", "epi_drop_act2",
        "epi_full", "rows_h0", "rows_h0_map", "rows_h4", "rows_h4_map", "bwd_act0", "bwd_act0_drop", "bwd_act1", "bwd_act1_drop", "bwd_act2",
        "bwd_act2_drop", "bwd_act3", "bwd_act3_drop", "bwd_act4", "bwd_act4_drop", "c_planes"),
    "x6tn": ("offsets", "tn_conv3", "tn_conv9", "split2_add", "split3_add", "split2_ow", "split3_ow", "split2_defer", "split3_defer", "epi_act0",
        "epi_act1", "epi_act2", "epi_act3", "epi_act4", "epi_res", "epi_drop", "epi_drop_act2", "epi_full", "rows_h0", "rows_h0_map", "rows_h4",
        "rows_h4_map"),
    "weight_stationary": ("offsets", "epi_act0", "epi_act1", "epi_act2", "epi_act4", "epi_drop_act2", "rows_h0_map", "rows_h4_map", "bwd_act0",
        "bwd_act0_drop", "bwd_act1", "bwd_act1_drop", "bwd_act2", "bwd_act2_drop", "bwd_act4", "bwd_act4_drop", "c_planes"),
    "planes": ("offsets", "conv3", "conv9", "split2_ow", "split3_ow", "epi_act0", "epi_act1", "epi_act2", "epi_act4", "epi_drop", "epi_drop_act2",
        "rows_h0", "rows_h0_map", "rows_h4", "rows_h4_map", "bwd_act2_drop", "bwd_act4_drop"),
    "planes_wgrad": ("offsets", "tn_conv3", "tn_conv9", "split2_add", "split3_add", "split2_ow", "split3_ow", "rows_h0", "rows_h0_map", "rows_h4",
        "rows_h4_map"),
    "stream_k": ("offsets", "conv3", "conv9", "tn_conv3", "tn_conv9", "split2_add", "split3_add", "split2_ow", "split3_ow", "epi_act0", "epi_act1",
        "epi_act2", "epi_act3", "epi_act4", "epi_res", "epi_drop", "epi_drop_act2", "epi_full", "rows_h0_map",
        "rows_h4_map", "bwd_act0", "bwd_act0_drop", "bwd_act1", "bwd_act1_drop", "bwd_act2", "bwd_act2_drop", "bwd_act3", "bwd_act3_drop", "bwd_act4",
        "bwd_act4_drop", "c_planes"),
}
# pairs whose feature fixes the layout to TN and whose kind does not take the EDGE shape in that layout: switched on at the BASE shape
BASE_SHAPED = {("buf_k2", "tn_conv3"), ("buf_k2", "tn_conv9"), ("stream_k", "tn_conv3"), ("stream_k", "tn_conv9")}


def _cases():
    out = []
    for kind in KINDS:
        for layout, M, N, Kd in SHAPES.get(kind, ()):
            out.append(Case(f"{kind}-{layout}-{M}x{N}x{Kd}", kind, layout, M, N, Kd, "shape", "exact"))
        for feat in FEATURES:
            layout, M, N, Kd = BASE[kind] if (kind, feat) in BASE_SHAPED else EDGE[kind]
            if feat in TAKES.get(kind, ()):
                out.append(Case(f"{kind}-{feat}", kind, layout, M, N, Kd, feat, "random" if feat in RANDOM else "exact"))
    return out


CASES = _cases()
