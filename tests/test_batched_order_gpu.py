"""GPU: the length-balanced tile order of the batched, length-limited attention products (csrc/batch_plan.h, kernels.batch_tile_map,
gemm_tile_kernel's Fetch::BufferPartial route).  The order changes where a tile runs, never what it computes: every product form of
ops._SelfAttention gives the same BITS with and without a plan over the whole NaN-filled output - the zeros of the "write everything"
rule and the cells nothing may write included - and agrees with float64; a captured graph that holds the plan build follows lengths
changed in place; _SelfAttention is bit-identical with the switch on and off."""
import pytest
import torch

import ctts_amd  # noqa: F401
from ctts_amd import kernels as K
from ctts_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None

B, H, T, dh = 6, 2, 192, 128
C, C3 = H * dh, 3 * H * dh
LENS = [192, 129, 65, 64, 1, 0]
SCALE = dh ** -0.5
S_TYPE, MAP_PRODUCT = ((1, 1, 0), False), ((1, 0, 1), True)          # lim, write_all (split_overwrite)


def heads(x, parts=1):
    return x.view(B, T, parts, H, dh).permute(2, 0, 3, 1, 4).unbind(0)


def bits(x):
    return x.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(11)
    d = dict(qkv=torch.randn(B, T, C3, generator=g), dO=torch.randn(B, T, C, generator=g), P=torch.rand(B, H, T, T, generator=g),
             dS=torch.randn(B, H, T, T, generator=g), Dv=torch.randn(B, H, T, generator=g))
    return {k: v.to(DEV) for k, v in d.items()}


def forms(d):
    """name -> (A, B, output slice of a fresh NaN buffer, geometry, keywords, float64 reference of one (b, h) cut at length L)"""
    q, k, v = heads(d["qkv"], 3)
    dOh, = heads(d["dO"])
    P, dS, Dv = d["P"], d["dS"], d["Dv"]
    tt = lambda: torch.full((B, H, T, T), float("nan"), device=DEV)
    packed = lambda i: heads(torch.full((B, T, C3), float("nan"), device=DEV), 3)[i]
    f64 = lambda x, b, h, L: x[b, h, :L].double()
    return {
        "S": (q, k.transpose(-1, -2), tt, S_TYPE, dict(alpha=SCALE),
              lambda b, h, L: SCALE * f64(q, b, h, L) @ f64(k, b, h, L).t()),
        "dP": (dOh, v.transpose(-1, -2), tt, S_TYPE, dict(E=P, rowsub=Dv),
               lambda b, h, L: P[b, h, :L, :L].double() * (f64(dOh, b, h, L) @ f64(v, b, h, L).t() - Dv[b, h, :L].double()[:, None])),
        "PV": (P, v, lambda: heads(torch.full((B, T, C), float("nan"), device=DEV))[0], MAP_PRODUCT, {},
               lambda b, h, L: P[b, h, :L, :L].double() @ f64(v, b, h, L)),
        "dV": (P.transpose(-1, -2), dOh, lambda: packed(2), MAP_PRODUCT, {},
               lambda b, h, L: P[b, h, :L, :L].double().t() @ f64(dOh, b, h, L)),
        "dK": (dS.transpose(-1, -2), q, lambda: packed(1), MAP_PRODUCT, dict(alpha=SCALE),
               lambda b, h, L: SCALE * dS[b, h, :L, :L].double().t() @ f64(q, b, h, L)),
        "dQ": (dS, k, lambda: packed(0), MAP_PRODUCT, dict(alpha=SCALE),
               lambda b, h, L: SCALE * dS[b, h, :L, :L].double() @ f64(k, b, h, L)),
    }


def launch(form, lens, plan):
    A, Bm, out, (lim, write_all), kw, _ = form
    Cout = out()
    K.bgemm(A, Bm, Cout, lens=lens, lim=lim, split_overwrite=write_all, tile_map=plan, **kw)
    return Cout


def plan_for(form, lens):
    A, Bm, _, (lim, write_all), _, _ = form
    plan = K.batch_tile_map(lens, H, A.shape[-2], Bm.shape[-1], A.shape[-1], lim, write_all)
    assert plan is not None
    return plan


@pytest.mark.parametrize("name", ["S", "dP", "PV", "dV", "dK", "dQ"])
def test_planned_launch_equals_plain_launch_and_float64(data, name):
    form = forms(data)[name]
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    plan = plan_for(form, lens)
    plain, planned = launch(form, lens, None), launch(form, lens, plan)
    torch.cuda.synchronize()
    hdr = plan[:4].tolist()
    tm = lambda L: -(-L // 64)
    n_active = sum(H * tm(L) * (tm(L) if form[3] is S_TYPE else dh // 64) for L in LENS)
    n_items = B * H * tm(T) * (tm(T) if form[3] is S_TYPE else dh // 64)
    assert hdr[:3] == [n_active, n_items if form[3][1] else n_active, n_items]
    assert sorted(plan[4:].tolist()) == [(z << 16) | t for z in range(B * H) for t in range(n_items // (B * H))]
    # storage-wide: the slices of the packed buffers the launch does not own stay NaN in both
    assert torch.equal(bits(planned._base if planned._base is not None else planned), bits(plain._base if plain._base is not None else plain))
    worst = 0.0
    for b, L in enumerate(LENS):
        for h in range(H):
            got = planned[b, h]
            if form[3] is S_TYPE:
                assert torch.isnan(got[L:]).all() and torch.isnan(got[:, L:]).all()      # nothing may be written there
                got = got[:L, :L]
            else:
                assert float(got[L:].abs().max()) == 0.0 if L < T else True             # "write everything"
                got = got[:L]
            if L:
                ref = form[5](b, h, L)
                worst = max(worst, float((got.double() - ref).abs().max() / ref.abs().max()))
    assert worst < 2e-6, worst          # the tolerance of tests/test_attention_products_gpu.py for these kernels


def test_a_plan_for_another_geometry_is_not_followed(data):
    """the kernel compares the plan's header with its own launch: a map-product launch handed an S-type plan runs in plain order"""
    f = forms(data)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    wrong = plan_for(f["S"], lens)
    assert torch.equal(bits(launch(f["PV"], lens, wrong)._base), bits(launch(f["PV"], lens, None)._base))


def test_plan_on_another_route_is_refused(data):
    f = forms(data)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    A, Bm, out, (lim, write_all), kw, _ = f["PV"]
    with pytest.raises(ctts_amd._lib.CttsError, match="batch tile plan"):
        K.bgemm(A, Bm, out(), lens=lens, lim=lim, split_k=2, split_overwrite=True, tile_map=plan_for(f["PV"], lens))


def test_captured_plan_build_follows_the_lengths(data):
    form = forms(data)["PV"]
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    A, Bm, _, (lim, write_all), kw, _ = form
    out = torch.empty(B, T, C, device=DEV)

    def run():
        plan = plan_for(form, lens)
        K.bgemm(A, Bm, heads(out)[0], lens=lens, lim=lim, split_overwrite=write_all, tile_map=plan, **kw)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
        run()
    for new in (LENS, [0, 192, 3, 191, 128, 127], [192] * 6):
        lens.copy_(torch.tensor(new, dtype=torch.int32))
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(launch(form, lens, None)._base)), new


def test_self_attention_is_bit_identical_with_the_switch(data, monkeypatch):
    Bs = 4
    qkv0, dO = data["qkv"][:Bs], data["dO"][:Bs].contiguous()
    lens = torch.tensor([192, 129, 65, 1], dtype=torch.int32, device=DEV)
    monkeypatch.setattr(ops, "_BATCH_ORDER_MIN_ITEMS", 0)        # these small launches would keep the plain order
    res = {}
    for order in ("balanced", "natural"):
        monkeypatch.setattr(ops, "_BATCH_ORDER", order)
        qkv = qkv0.clone().requires_grad_(True)
        pr = ops.PadRows(lens, T)
        out = ops._SelfAttention.apply(qkv, lens, H, pr)
        dqkv, = torch.autograd.grad(out, qkv, dO)
        assert len(pr._batch_maps) == (2 if order == "balanced" else 0)          # one plan per geometry, shared by forward and backward
        assert all(p is not None for p in pr._batch_maps.values())
        res[order] = (out.detach(), dqkv)
    torch.cuda.synchronize()
    assert torch.equal(bits(res["balanced"][0]), bits(res["natural"][0]))
    assert torch.equal(bits(res["balanced"][1]), bits(res["natural"][1]))
