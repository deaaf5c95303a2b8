"""ctts_gemm_route (csrc/gemm.hip gemm_route): which kernel family takes a GEMM descriptor.  Host code only - the pointers are made up, no
query dereferences them - so the table below runs without a GPU: the model's own launches and the edges between the families.

The expected kinds of the tile-kernel rows (scalar64, buf64, buf_k2, buf_narrow, vec64) come from reading the kernel choice of ctts_gemm
as it stood before the routing function existed (the `K_*` enum of gemm_impl); the rows of the other families are what the public
queries answered then.  On every row the public queries must agree with the route the way include/ctts.h says they do."""
import ctypes as C
import os
import re

import pytest

import ctts_amd  # noqa: F401
from ctts_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 0x7F0000000000          # made-up, 16-byte aligned "device" addresses, 64 GiB apart


def _ptr(i):
    return BASE + i * (1 << 36)


def _desc(M, N, K, layout="NT", lda=None, ws=False, planes=False, conv=None, conv_on_b=False, **fields):
    d = _lib.GemmDesc()
    d.a_kc, d.b_kc = {"NT": (1, 1), "NN": (1, 0), "TN": (0, 0)}[layout]
    d.M, d.N, d.K = M, N, K
    d.lda = lda if lda is not None else (K if d.a_kc else M)
    d.ldb = K if d.b_kc else N
    d.ldc = N
    d.A, d.B, d.C = _ptr(1), _ptr(2), _ptr(3)
    d.nb0 = d.nb1 = 1
    d.alpha = 1.0
    if ws:
        d.sk_ws, d.sk_ws_bytes = _ptr(4), _lib.load().ctts_workspace_bytes()
    if planes:
        d.A_planes, d.B_planes = _ptr(5), _ptr(6)
    if conv is not None:
        d.conv_T, d.conv_pad, d.conv_cin = conv
        d.conv_on_b = int(conv_on_b)
    for k, v in fields.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    return d


# (id, descriptor, kind, (tile_m, tile_n), split_k, k_granule, split plan or None)
ROWS = [
    ("unaligned_K", _desc(70, 50, 30), "scalar64", (64, 64), 1, 32, None),
    ("small_two_tiles", _desc(130, 130, 64), "buf64", (64, 64), 1, 32, None),
    ("few_tiles_k2", _desc(256, 64, 256), "buf_k2", (32, 64), 1, 64, None),
    ("narrow_output", _desc(256, 32, 64), "buf_narrow", (128, 32), 1, 32, None),
    ("x6_forced", _desc(1024, 128, 256, bf16_split=2), "x6", (128, 128), 1, 32, None),
    ("x6tn_split2", _desc(128, 128, 2048, "TN", ws=True, split_k=2, bf16_split=2), "x6tn", (128, 128), 2, 32, (2, 16384)),
    ("ws_64_columns", _desc(4096, 64, 256), "weight_stationary", (64, 128), 1, 32, None),
    ("planes_small", _desc(128, 256, 64, ws=True, planes=True, bf16_split=2), "planes", (128, 256), 1, 32, None),
    ("planes_wgrad_small", _desc(128, 256, 64, "TN", ws=True, planes=True, bf16_split=2, split_k=2), "planes_wgrad", (128, 256), 1, 32, None),
    ("stream_k_NT", _desc(4096, 1024, 2048, "NT", ws=True, bf16_split=0), "stream_k", (128, 128), 1, 32, None),
    ("stream_k_NN", _desc(4096, 1024, 2048, "NN", ws=True, bf16_split=0), "stream_k", (128, 128), 1, 32, None),
    ("stream_k_TN", _desc(4096, 1024, 2048, "TN", ws=True, bf16_split=0), "stream_k", (128, 128), 1, 32, None),
    ("operand_past_2GiB", _desc(4096, 256, 256, lda=1 << 18), "vec64", (64, 64), 1, 32, None),
    ("decoder_ffn_conv_fwd", _desc(16384, 1024, 2304, ws=True, planes=True, conv=(1024, 4, 256), bf16_split=1), "planes", (128, 256), 1, 32, None),
    ("attention_out_linear", _desc(16384, 768, 256), "weight_stationary", (64, 128), 1, 32, None),
    ("wgrad_split8", _desc(256, 1024, 16384, "TN", ws=True, split_k=8, bf16_split=1), "buf_k2", (32, 64), 8, 64, (8, 262144)),
]


def _route(d):
    info = _lib.GemmRouteInfo()
    rc = _lib.load().ctts_gemm_route(C.byref(d), C.byref(info))
    return rc, info


@pytest.mark.parametrize("name,d,kind,tile,split_k,granule,plan", ROWS, ids=[r[0] for r in ROWS])
def test_route_table(name, d, kind, tile, split_k, granule, plan):
    lib = _lib.load()
    rc, info = _route(d)
    assert rc == 0, lib.ctts_last_error()
    got = _lib.GEMM_KINDS[info.kind]
    assert (got, (info.tile_m, info.tile_n), info.split_k, info.k_granule) == (kind, tile, split_k, granule)
    # the public queries against the route (include/ctts.h)
    assert lib.ctts_gemm_takes_planes(C.byref(d)) == int(got in ("planes", "planes_wgrad"))
    assert lib.ctts_gemm_takes_bf16_split(C.byref(d)) == int(got in ("x6", "x6tn"))
    if got == "stream_k":
        assert lib.ctts_gemm_takes_persistent(C.byref(d)) == 1
    if got == "weight_stationary":
        assert lib.ctts_gemm_takes_weight_stationary(C.byref(d)) == 1
    cnt, stride = C.c_int32(0), C.c_int64(0)
    said = lib.ctts_gemm_split_plan(C.byref(d), C.byref(cnt), C.byref(stride))
    assert said == int(plan is not None)
    if said:
        chunk = -(-(-(-d.K // info.split_k)) // info.k_granule) * info.k_granule
        assert (cnt.value, stride.value) == (-(-d.K // chunk), d.M * (-(-d.N // 4) * 4)) == plan


def test_persistent_and_weight_stationary_answer_for_themselves():
    """ops relies on takes_persistent meaning "eligible when asked alone": the decoder FFN conv forward runs on the plane kernel and is
    eligible for stream-K as well"""
    lib = _lib.load()
    d = dict((r[0], r[1]) for r in ROWS)["decoder_ffn_conv_fwd"]
    assert lib.ctts_gemm_takes_planes(C.byref(d)) == 1 and lib.ctts_gemm_takes_persistent(C.byref(d)) == 1


def test_route_validates_like_the_launch():
    lib = _lib.load()
    d = _desc(130, 130, 64)
    d.A = None
    rc, info = _route(d)
    assert rc < 0 and b"null operand" in lib.ctts_last_error() and info.kind == 0
    rc, _ = _route(_desc(256, 1024, 16384, "TN", split_k=8))          # split-K partials need the workspace
    assert rc < 0 and b"workspace" in lib.ctts_last_error()
    rc, _ = _route(_desc(64, 64, 64, "NT", conv=(16, 1, 6)))
    assert rc < 0 and b"cin" in lib.ctts_last_error()
    rc, info = _route(_desc(0, 64, 64))                               # empty output: no error, nothing to launch
    assert rc == 0 and _lib.GEMM_KINDS[info.kind] == "none"


def test_kind_names_follow_the_header_enum():
    text = open(os.path.join(ROOT, "include", "ctts.h")).read()
    body = re.search(r"typedef enum ctts_gemm_kind \{(.*?)\} ctts_gemm_kind;", text, re.S).group(1)
    names = re.findall(r"CTTS_GEMM_([A-Z0-9_]+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert tuple(n.lower() for n in names) == _lib.GEMM_KINDS
    assert "ctts_gemm_route" in _lib.EXPORTED_SYMBOLS


def test_stale_library_is_refused_at_load(monkeypatch):
    assert _lib.load().ctts_version() == _lib.ABI_VERSION == 2
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "ABI_VERSION", 3)
    with pytest.raises(_lib.CttsError, match="ABI version"):
        _lib.load()
