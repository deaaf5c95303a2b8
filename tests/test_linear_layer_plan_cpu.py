"""CPU: the launch plan of ops.linear / ops.conv1d (ops._LinearConv), observed through recording stand-ins for the kernel wrappers - the
operator itself runs on CPU tensors once nothing is launched.  Pinned here: every eligibility query describes the launch it decides
about, gradient-accumulation fusion hands the kernels `param.grad`, the EpiLink hand-off, and the program order of dropout offsets.
Numerics are held by the GPU tests; nothing here computes a value."""
import inspect

import pytest
import torch

import ctts_amd  # noqa: F401
from ctts_amd import kernels as K
from ctts_amd import ops

PLANE_KEYS = ("a_planes", "b_planes", "c_planes")
# what an absent keyword means to the descriptor (kernels._gemm_desc); `defer` is K.gemm's own argument: how split-K partials are summed
DESC_DEFAULTS = {n: p.default for n, p in inspect.signature(K._gemm_desc).parameters.items() if p.default is not inspect.Parameter.empty}


class Recorder:
    """stand-ins for the kernel wrappers: record (name, args, kw), return tensors of the right shape, launch nothing"""

    def __init__(self, monkeypatch, takes):
        self.calls, self.takes = [], {"planes": False, "persistent": False, "weight_stationary": False, **takes}
        for name in ("gemm", "split_planes", "conv_weight_repack", "colsum", "weighted_colsum", "epilogue_bwd", "row_tile_map"):
            monkeypatch.setattr(K, name, getattr(self, name))
        for what in ("planes", "persistent", "weight_stationary"):
            monkeypatch.setattr(K, "gemm_takes_" + what, self._query(what))
        for flag in ("PLANES_ENABLED", "PLW_ENABLED", "SK_ENABLED"):
            monkeypatch.setattr(K, flag, True)
        monkeypatch.setattr(K, "BF16_SPLIT", 2)          # the plane pre-filters pass at small shapes

    def _query(self, what):
        def ask(*args, **kw):
            self.calls.append(("takes_" + what, args, kw, self.takes[what]))
            return self.takes[what]
        return ask

    def gemm(self, *args, **kw):
        self.calls.append(("gemm", args, kw))
        return args[2]

    def split_planes(self, mats):
        self.calls.append(("split_planes", tuple(mats), {}))
        return [torch.empty(m.shape[0], m.shape[1] // 32, 3, 32, dtype=torch.bfloat16) for m in mats]

    def conv_weight_repack(self, src, dst, cout, cin, k, mode):
        self.calls.append(("conv_weight_repack", (src, dst, cout, cin, k, mode), {}))
        return dst

    def colsum(self, x2d, ld=None, scale=1.0, acc_into=None):
        self.calls.append(("colsum", (x2d,), dict(scale=scale, acc_into=acc_into)))
        return acc_into if acc_into is not None else torch.zeros(x2d.shape[1])

    def weighted_colsum(self, x2d, w, scale=1.0, acc_into=None):
        self.calls.append(("weighted_colsum", (x2d, w), dict(scale=scale, acc_into=acc_into)))
        return acc_into if acc_into is not None else torch.zeros(x2d.shape[1])

    def epilogue_bwd(self, dy, rowscale=None, z=None, act=0, p_drop=0.0, seed=None, drop_offset=0, want_gm=False, want_bias=False,
                     bias_scale=1.0, bias_acc_into=None):
        self.calls.append(("epilogue_bwd", (dy,), dict(want_bias=want_bias, bias_scale=bias_scale, bias_acc_into=bias_acc_into)))
        dB = (bias_acc_into if bias_acc_into is not None else torch.zeros(dy.shape[-1])) if want_bias else None
        return torch.zeros_like(dy), (torch.zeros_like(dy) if want_gm else None), dB

    def row_tile_map(self, row_lens, row_T, row_halo, M):
        self.calls.append(("row_tile_map", (row_lens, row_T, row_halo, M), {}))
        return torch.zeros(1 + (M + 63) // 64, dtype=torch.int32)

    def named(self, name):
        return [c for c in self.calls if c[0] == name]


@pytest.fixture
def rec(monkeypatch):
    fusion = ops.grad_accumulation_fusion()
    want = {k: set(v) for k, v in ops._PLANES.items() if k.startswith("want_")}
    made = []

    def make(**takes):
        made.append(Recorder(monkeypatch, takes))
        return made[-1]
    yield make
    ops.set_grad_accumulation_fusion(fusion)
    ops._PLANES.update(want)


class Drop:
    """kernels.DropCtx without a device"""

    def __init__(self):
        self.seed, self.counter = torch.zeros(1, dtype=torch.int64), 0

    def next_offset(self):
        self.counter += 1
        return self.counter


def gemm_major(cout, cin, k):
    """a Conv1d weight in the memory layout of model._Conv: shape [Cout, Cin, k], memory [Cout][k][Cin]"""
    return torch.nn.Parameter((torch.randn(cout, k, cin) * 0.02).permute(0, 2, 1))


def conv_layer(cin, cout, k, B=2, T=128, pad_rows=True, w=None):
    x = torch.randn(B, T, cin, requires_grad=True)
    w = gemm_major(cout, cin, k) if w is None else w
    b = torch.nn.Parameter(torch.zeros(cout))
    pr = ops.PadRows(torch.tensor([T, T // 2], dtype=torch.int32), T) if pad_rows else None
    y = ops.conv1d(x, w, b, act=ops.ACT_GELU, p_drop=0.1, drop=Drop(), pad_rows=pr)
    return x, w, b, y


def same(a, b):
    return a is b or (not torch.is_tensor(a) and not torch.is_tensor(b) and a == b)


def assert_queries_describe_their_launches(calls, expect):
    """every query that was answered yes is followed by the K.gemm call it decided about, with the same descriptor"""
    seen = []
    for i, (name, args, kw, *answer) in enumerate(calls):
        if answer != [True]:
            continue
        nxt = next(c for c in calls[i + 1:] if c[0] == "gemm" or c[0].startswith("takes_"))
        seen.append(name)
        assert nxt[0] == "gemm", f"{name} answered yes and no launch followed"
        largs, lkw = nxt[1], nxt[2]
        assert largs[2] is args[2], f"{name}: asked about another output tensor than the launch writes"
        assert largs[0].data_ptr() == args[0].data_ptr() and largs[1].data_ptr() == args[1].data_ptr(), f"{name}: operand addresses"
        assert tuple(largs[3:]) == tuple(args[3:]), f"{name}: dims / layout flags {args[3:]} vs launch {largs[3:]}"
        q, launch = ({**DESC_DEFAULTS, **{k: v for k, v in d.items() if k not in PLANE_KEYS and k != "defer"}} for d in (kw, lkw))
        diff = sorted(k for k in q if not same(q[k], launch[k]))
        assert not diff, f"{name}: keywords differ between query and launch: " + ", ".join(f"{k}={q[k]!r}/{launch[k]!r}" for k in diff)
        for k in PLANE_KEYS:
            assert (kw.get(k) is None) == (lkw.get(k) is None), f"{name}: {k} asked for and not launched with (or the reverse)"
    assert seen == expect


@pytest.mark.parametrize("pad_rows", [False, True])
def test_plane_queries_are_asked_with_the_arguments_of_their_launch(rec, pad_rows):
    """forward, data-gradient and weight-gradient plane queries: Cin = Cout = 256, k = 3, B = 2, T = 128"""
    r = rec(planes=True)
    x, w, b, y = conv_layer(256, 256, 3, pad_rows=pad_rows)
    y.sum().backward()
    assert_queries_describe_their_launches(r.calls, ["takes_planes"] * 3)
    fwd, dgrad, wgrad = r.named("gemm")
    assert all(g[2].get("a_planes") is not None and g[2].get("b_planes") is not None for g in (fwd, dgrad, wgrad))
    assert fwd[2].get("tile_map") is None and dgrad[2].get("tile_map") is None          # the plane kernels walk no m-tile schedule
    # plane reuse: the weight gradient reads dZ's set of the data-gradient launch and x's set of the forward launch; only the two
    # activations and the two weight matrices were ever split
    assert wgrad[2]["a_planes"] is dgrad[2]["a_planes"] and wgrad[2]["b_planes"] is fwd[2]["a_planes"]
    assert sum(len(c[1]) for c in r.named("split_planes")) == 4


def test_persistent_query_is_asked_with_the_arguments_of_its_launch(rec):
    """planes decline; Cin = 256, Cout = 1024, k = 9 gives 16 data-gradient tiles and split_k 4, so the stream-K kernel is asked - about
    dX and split_overwrite=True, which is what the launch that follows writes"""
    r = rec(persistent=True)
    x, w, b, y = conv_layer(256, 1024, 9)
    y.sum().backward()
    assert_queries_describe_their_launches(r.calls, ["takes_persistent"])
    q = r.named("takes_persistent")[0]
    assert q[2]["split_overwrite"] is True and q[2]["split_k"] == 1 and q[1][2] is not x and q[1][2].shape == x.shape


def test_data_gradient_is_split_when_the_persistent_kernel_declines(rec):
    r = rec()
    x, w, b, y = conv_layer(256, 1024, 9)
    y.sum().backward()
    assert len(r.named("takes_persistent")) == 1
    dgrad = r.named("gemm")[1]
    assert dgrad[2]["split_k"] == 4 and dgrad[2]["split_overwrite"] is True and dgrad[2]["tile_map"] is not None


def _storage(t):
    return t.untyped_storage().data_ptr()


def _layers():
    def lin():
        w = torch.nn.Parameter(torch.randn(48, 32))
        return w, lambda x, b: ops.linear(x, w, b), 32

    def conv_contiguous():
        w = torch.nn.Parameter(torch.randn(48, 32, 3))
        return w, lambda x, b: ops.conv1d(x, w, b, act=ops.ACT_RELU), 32

    def conv_gemm_major():
        w = gemm_major(48, 32, 3)
        return w, lambda x, b: ops.conv1d(x, w, b, act=ops.ACT_RELU), 32
    return [lin, conv_contiguous, conv_gemm_major]


@pytest.mark.parametrize("layer", _layers(), ids=lambda f: f.__name__)
def test_fused_accumulation_hands_the_kernels_param_grad_and_autograd_none(rec, layer):
    r = rec()
    w, fn, cin = layer()
    b = torch.nn.Parameter(torch.zeros(48))
    w.grad, b.grad = torch.zeros_like(w), torch.zeros_like(b)          # zeros_like keeps the GEMM-major strides
    assert w.grad.stride() == w.stride()
    x = torch.randn(2, 40, cin, requires_grad=True)

    ops.set_grad_accumulation_fusion(True)
    dx, dw, db = torch.autograd.grad(fn(x, b).sum(), [x, w, b], allow_unused=True)
    assert dx is not None and dw is None and db is None
    wgrad = r.named("gemm")[-1]
    repack = [c for c in r.named("conv_weight_repack") if c[1][5] == 3]
    if layer.__name__ == "conv_contiguous":          # GEMM-major scratch matrix, repacked (mode 3: accumulate) into param.grad
        assert len(repack) == 1 and repack[0][1][0] is wgrad[1][2] and repack[0][1][1] is w.grad
        assert wgrad[2]["split_overwrite"] is True and not wgrad[2].get("defer")
    else:                                            # the split-K partials are added straight into param.grad
        assert not repack and _storage(wgrad[1][2]) == _storage(w.grad) and wgrad[1][2].data_ptr() == w.grad.data_ptr()
        assert not wgrad[2].get("split_overwrite") and wgrad[2]["defer"] is True
    sums = [c[2]["acc_into"] for c in r.named("colsum")] + [c[2]["bias_acc_into"] for c in r.named("epilogue_bwd") if c[2]["want_bias"]]
    assert len(sums) == 1 and sums[0].data_ptr() == b.grad.data_ptr() and _storage(sums[0]) == _storage(b.grad)

    ops.set_grad_accumulation_fusion(False)
    r.calls.clear()
    dx, dw, db = torch.autograd.grad(fn(x, b).sum(), [x, w, b], allow_unused=True)
    assert dw.shape == w.shape and db.shape == b.shape
    wgrad = r.named("gemm")[-1]
    assert _storage(wgrad[1][2]) != _storage(w.grad) and wgrad[2]["split_overwrite"] is True and not wgrad[2].get("defer")
    sums = [c[2]["acc_into"] for c in r.named("colsum")] + [c[2]["bias_acc_into"] for c in r.named("epilogue_bwd") if c[2]["want_bias"]]
    assert sums == [None]
    if layer.__name__ == "conv_gemm_major":          # a view of the GEMM result with the parameter's own strides: no repack
        assert dw.stride() == w.stride() and _storage(dw) == _storage(wgrad[1][2])


def test_one_output_head_is_a_weighted_column_sum_unless_rows_are_ragged(rec):
    r = rec()
    w = torch.nn.Parameter(torch.randn(1, 32))
    x = torch.randn(2, 40, 32, requires_grad=True)
    ops.linear(x, w).sum().backward()
    assert len(r.named("weighted_colsum")) == 1 and len(r.named("gemm")) == 2          # forward, data gradient
    r.calls.clear()
    ops.linear(x, w, pad_rows=(torch.tensor([40, 7], dtype=torch.int32), 40)).sum().backward()
    assert not r.named("weighted_colsum") and len(r.named("gemm")) == 3


def _ffn(rec_, fuse_epi, monkeypatch):
    monkeypatch.setattr(ops, "_FUSE_EPILOGUE_BWD", fuse_epi)
    r = rec_()
    drop, link = Drop(), ops.EpiLink()
    x = torch.randn(2, 40, 32, requires_grad=True)
    w1, b1 = gemm_major(64, 32, 3), torch.nn.Parameter(torch.zeros(64))
    w2, b2 = torch.nn.Parameter(torch.randn(32, 64)), torch.nn.Parameter(torch.zeros(32))
    h = ops.conv1d(x, w1, b1, act=ops.ACT_GELU, alpha=0.5, p_drop=0.1, drop=drop, link=link, link_role=1)
    y = ops.linear(h, w2, b2, link=link, link_role=2)
    n_fwd = len(r.calls)
    y.sum().backward()
    return r, r.calls[n_fwd:], drop, link


def test_epilink_consumer_applies_the_producer_epilogue_backward(rec, monkeypatch):
    r, bwd, drop, link = _ffn(rec, True, monkeypatch)
    producer_fwd = r.named("gemm")[0][2]
    assert producer_fwd["Z"] is not None and producer_fwd["drop_offset"] == 1
    gemms = [c for c in bwd if c[0] == "gemm"]
    dgrad = gemms[0]                         # the consumer's data gradient is the first launch of the backward pass
    kw = dgrad[2]
    assert kw["epi_bwd"] is True and kw["Z"] is producer_fwd["Z"] and kw["act"] == ops.ACT_GELU and kw["p_drop"] == 0.1
    assert kw["seed"] is drop.seed and kw["drop_offset"] == 1 and kw["ldz"] == 64
    assert not [c for c in bwd if c[0] == "epilogue_bwd"]          # the producer runs no separate pass over its [M, N] gradient ...
    sums = [c for c in bwd if c[0] == "colsum"]
    assert len(sums) == 2                                            # ... and still sums its bias: alpha * colsum(dZ), dZ = the consumer's dX
    assert sums[1][1][0].data_ptr() == dgrad[1][2].data_ptr() and sums[1][2]["scale"] == 0.5
    assert not link.done and not link.armed


def test_epilink_switched_off_brings_the_separate_epilogue_pass_back(rec, monkeypatch):
    r, bwd, drop, link = _ffn(rec, False, monkeypatch)
    assert not any(c[2].get("epi_bwd") for c in bwd if c[0] == "gemm")
    epi = [c for c in bwd if c[0] == "epilogue_bwd"]
    assert len(epi) == 1 and epi[0][2]["want_bias"] and epi[0][2]["bias_scale"] == 0.5
    assert len([c for c in bwd if c[0] == "colsum"]) == 1            # the consumer's own bias


def test_dropout_offsets_follow_program_order_and_are_drawn_only_by_layers_that_drop(rec):
    r = rec()
    drop = Drop()
    x = torch.randn(2, 40, 32)
    w, wc = torch.randn(32, 32), torch.randn(32, 32, 3)
    h = ops.linear(x, w, p_drop=0.1, drop=drop)
    h = ops.conv1d(h, wc, p_drop=0.0, drop=drop)          # p_drop == 0: draws nothing
    h = ops.conv1d(h, wc, p_drop=0.2, drop=drop)
    h = ops.linear(h, w, p_drop=0.5, drop=None)           # no DropCtx: no dropout
    h = ops.linear(h, w, act=ops.ACT_RELU, p_drop=0.3, drop=drop)
    got = [(c[2]["p_drop"], c[2]["seed"] is drop.seed, c[2]["drop_offset"]) for c in r.named("gemm")]
    assert got == [(0.1, True, 1), (0.0, False, 0), (0.2, True, 2), (0.0, False, 0), (0.3, True, 3)]
    assert drop.counter == 3
