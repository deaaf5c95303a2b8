"""CPU: pins tests/gemm_restate64.py (the float64 restatement of ctts_gemm_desc that tests/test_gemm_contract_gpu.py compares the kernels
with) against torch compositions in float64, one per descriptor feature, and checks the case table of tests/gemm_cases.py against
ctts_gemm_route: every row's kind, tile and granule, and the completeness of the (kind, feature) list.  No GPU: the route query is host
code and dereferences nothing."""
import pytest
import torch
import torch.nn.functional as F

import ctts_amd  # noqa: F401
from ctts_amd import _lib
from tests import gemm_cases as G
from tests import gemm_restate64 as R64
from tests.attention_restate import attention_keep_mask

D = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _r(g, *shape):
    return torch.rand(*shape, generator=g, dtype=D) * 2 - 1


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_linear_with_offsets_and_padded_leading_dimensions_leaves_every_other_cell_alone():
    g = _g(1)
    M, N, Kd, lda, ldb, ldc, a_off, b_off, c_off = 7, 5, 6, 9, 8, 11, 3, 2, 13
    A, B, bias = _r(g, a_off + M * lda), _r(g, b_off + N * ldb), _r(g, N)
    C0 = _r(g, c_off + M * ldc + 4)
    out = R64.restate(A, B, C0, M, N, Kd, lda, ldb, ldc, True, True, a_off=a_off, b_off=b_off, c_off=c_off, alpha=0.3, bias=bias)
    x = A[a_off:a_off + M * lda].view(M, lda)[:, :Kd]
    w = B[b_off:b_off + N * ldb].view(N, ldb)[:, :Kd]
    want = C0.clone()
    want[c_off:c_off + M * ldc].view(M, ldc)[:, :N] = 0.3 * F.linear(x, w, bias)
    _close(out.C, want)
    assert int(out.written_C.sum()) == M * N and torch.equal(out.C[~out.written_C], C0[~out.written_C])
    # NN and TN read the same numbers through the other layouts
    Bt = torch.zeros(Kd * ldb, dtype=D)
    Bt.view(Kd, ldb)[:, :N] = w.t()
    _close(R64.restate(A, Bt, C0, M, N, Kd, lda, ldb, ldc, True, False, a_off=a_off, c_off=c_off, alpha=0.3, bias=bias).C, want)
    At = torch.zeros(Kd * lda, dtype=D)
    At.view(Kd, lda)[:, :M] = x.t()
    _close(R64.restate(At, Bt, C0, M, N, Kd, lda, ldb, ldc, False, False, c_off=c_off, alpha=0.3, bias=bias).C, want)


@pytest.mark.parametrize("k", [3, 9])
def test_conv_view_on_a_is_conv1d_with_same_padding_on_channel_last_data(k):
    g = _g(2)
    B_, T, cin, cout = 3, 7, 4, 5
    x, w = _r(g, B_, T, cin), _r(g, cout, cin, k)
    wf = w.permute(0, 2, 1).reshape(cout, k * cin)                  # [cout][k][cin]
    C0 = torch.zeros(B_ * T * cout, dtype=D)
    out = R64.restate(x, wf, C0, B_ * T, cout, k * cin, cin, k * cin, cout, True, True, conv=(T, k // 2, cin))
    want = F.conv1d(x.transpose(1, 2), w, padding=k // 2).transpose(1, 2)
    _close(out.C.view(B_, T, cout), want)


@pytest.mark.parametrize("k", [3, 9])
def test_conv_view_on_b_is_autograds_weight_gradient_of_conv1d(k):
    g = _g(3)
    B_, T, cin, cout = 2, 8, 4, 3
    x, dz = _r(g, B_, T, cin), _r(g, B_, T, cout)
    w = _r(g, cout, cin, k).requires_grad_()
    (F.conv1d(x.transpose(1, 2), w, padding=k // 2).transpose(1, 2) * dz).sum().backward()
    want = w.grad.permute(0, 2, 1).reshape(cout, k * cin)
    C0 = torch.ones(cout * k * cin, dtype=D)
    out = R64.restate(dz, x, C0, cout, k * cin, B_ * T, cout, cin, k * cin, False, False, conv=(T, k // 2, cin), conv_on_b=True,
                      split_k=2, alpha=0.5)
    _close(out.C.view(cout, k * cin), 1.0 + 0.5 * want)            # split_k > 1 adds into C


def test_two_batch_levels_with_length_limits_are_masked_bmm():
    g = _g(4)
    nb0, nb1, T, dh = 3, 2, 6, 4
    q, kk, v = _r(g, nb0, nb1, T, dh), _r(g, nb0, nb1, T, dh), _r(g, nb0, nb1, T, dh)
    lens = torch.tensor([1, 6, 4], dtype=torch.int32)
    sA = (nb1 * T * dh, T * dh)
    sC = (nb1 * T * T, T * T)
    C0 = torch.full((nb0 * nb1 * T * T,), 7.0, dtype=D)
    for ow in (False, True):
        out = R64.restate(q, kk, C0, T, T, dh, dh, dh, T, True, True, nb0=nb0, nb1=nb1, sA=sA, sB=sA, sC=sC, lens=lens, lim=(1, 1, 0),
                          alpha=0.25, split_overwrite=ow)
        S = out.C.view(nb0, nb1, T, T)
        for b in range(nb0):
            L = int(lens[b])
            _close(S[b, :, :L, :L], 0.25 * torch.bmm(q[b, :, :L], kk[b, :, :L].transpose(1, 2)))
            rest = torch.ones(T, T, dtype=torch.bool)
            rest[:L, :L] = False
            assert bool((S[b][:, rest] == (0.0 if ow else 7.0)).all())
    # lim_k: P[:, :L] @ V[:L] (NN)
    P = _r(g, nb0, nb1, T, T)
    out = R64.restate(P, v, torch.zeros(nb0 * nb1 * T * dh, dtype=D), T, dh, T, T, dh, dh, True, False, nb0=nb0, nb1=nb1,
                      sA=(nb1 * T * T, T * T), sB=sA, sC=sA, lens=lens, lim=(0, 0, 1))
    for b in range(nb0):
        L = int(lens[b])
        _close(out.C.view(nb0, nb1, T, dh)[b], torch.bmm(P[b, :, :, :L], v[b, :, :L]))


@pytest.mark.parametrize("code,fn", [(0, lambda v: v), (1, F.relu), (2, F.gelu), (3, torch.tanh), (4, F.silu)])
def test_forward_epilogue_and_its_backward_against_torch_activations_and_autograd(code, fn):
    g = _g(5)
    M, N, Kd, p = 6, 5, 4, 0.25
    A, B, bias, R, rs = _r(g, M, Kd), _r(g, N, Kd), _r(g, N), _r(g, M, N), (torch.rand(M, generator=g) > 0.3).to(D)
    seed = torch.tensor([0x123456789ABCDEF], dtype=torch.int64)
    keep = R64.keep_mask(int(seed[0]), 9, p, (torch.arange(M)[:, None] * N + torch.arange(N)[None, :]).numpy())
    # the attention restatement numbers a [T, T] map row-major; the epilogue numbers [M, N] as m * N + n: the same for T = N
    assert torch.equal(keep[:N], attention_keep_mask(int(seed[0]), 9, p, 1, 1, N)[0, 0])
    assert 0.4 < float(keep.double().mean()) < 0.98
    Z0 = torch.zeros(M * N, dtype=D)
    out = R64.restate(A, B, torch.zeros(M * N, dtype=D), M, N, Kd, Kd, Kd, N, True, True, alpha=0.7, bias=bias, Z=Z0, ldz=N, act=code,
                      p_drop=p, seed=seed, drop_offset=9, R=R, ldr=N, rowscale=rs)
    z = 0.7 * (F.linear(A, B) + bias)
    _close(out.Z.view(M, N), z)
    _close(out.C.view(M, N), rs[:, None] * (R + fn(z) * keep.to(D) / (1 - p)))
    assert torch.equal(out.dropped_C.view(M, N), ~keep)
    # backward: C = mask / (1 - p) * act'(Z) * alpha * acc, act' from autograd
    zz = _r(g, M, N).requires_grad_()
    fn(zz).sum().backward()
    dact = zz.grad if code else torch.ones(M, N, dtype=D)
    outb = R64.restate(A, B, torch.zeros(M * N, dtype=D), M, N, Kd, Kd, Kd, N, True, True, alpha=0.7, Z=zz.detach() if code else None, ldz=N,
                       act=code, p_drop=p, seed=seed, drop_offset=9, epi_bwd=True)
    _close(outb.C.view(M, N), keep.to(D) / (1 - p) * dact * 0.7 * F.linear(A, B))
    if code:
        assert not bool(outb.written_Z.any()) and torch.equal(outb.Z, zz.detach().reshape(-1))      # Z is an input


def test_e_rowsub_is_the_softmax_backward_identity():
    g = _g(6)
    nb, T, dh = 2, 5, 3
    S = _r(g, nb, T, T).requires_grad_()
    V, dO = _r(g, nb, T, dh), _r(g, nb, T, dh)
    P = torch.softmax(S, -1)
    O = P @ V
    (O * dO).sum().backward()
    rowsub = (dO * O.detach()).sum(-1).reshape(-1)
    c_off = 3
    C0 = torch.zeros(c_off + nb * T * T, dtype=D)
    out = R64.restate(dO, V, C0, T, T, dh, dh, dh, T, True, True, c_off=c_off, nb0=nb, nb1=1, sA=(T * dh, 0), sB=(T * dh, 0), sC=(T * T, 0),
                      E=P.detach(), rowsub=rowsub)
    _close(out.C[c_off:].view(nb, T, T), S.grad)


def test_split_k_adds_overwrites_or_leaves_its_partials_in_the_plan_layout():
    g = _g(7)
    M, N, Kd = 5, 6, 200
    A, B = _r(g, Kd, M), _r(g, Kd, N)
    C0 = _r(g, M * N)
    prod = A.t() @ B
    add = R64.restate(A, B, C0, M, N, Kd, M, N, N, False, False, split_k=3, alpha=0.5)
    _close(add.C.view(M, N), C0.view(M, N) + 0.5 * prod)
    ow = R64.restate(A, B, C0, M, N, Kd, M, N, N, False, False, split_k=3, alpha=0.5, split_overwrite=True)
    _close(ow.C.view(M, N), 0.5 * prod)
    # the K ranges of gemm_split_range (csrc/gemm_common.h): equal chunks, rounded up to the granule, trailing pieces may be empty
    assert R64.split_ranges(200, 3, 32) == [(0, 96), (96, 192), (192, 200)]
    assert R64.split_ranges(200, 3, 64) == [(0, 128), (128, 200)]
    assert R64.split_ranges(64, 3, 32) == [(0, 32), (32, 64)]
    ldp, stride = 8, M * 8
    P0 = torch.full((3 * stride + 5,), -3.0, dtype=D)
    de = R64.restate(A, B, C0, M, N, Kd, M, N, N, False, False, split_k=3, alpha=0.5, split_out=P0, split_plan=(3, stride), k_granule=32)
    assert torch.equal(de.C, C0) and not bool(de.written_C.any())
    parts = de.split_out[:3 * stride].view(3, M, ldp)
    _close(parts[:, :, :N].sum(0), prod)
    assert bool((parts[:, :, N:] == -3.0).all()) and bool((de.split_out[3 * stride:] == -3.0).all())
    assert int(de.written_split.sum()) == 3 * M * N


def test_padded_rows_are_zero_and_the_operands_must_make_them_so():
    g = _g(8)
    T, Kd, N = 6, 4, 3
    lens = torch.tensor([2, 6, 1], dtype=torch.int32)
    M = 3 * T
    A, B = _r(g, M, Kd), _r(g, N, Kd)
    C0 = torch.full((M * N,), 9.0, dtype=D)
    with pytest.raises(ValueError, match="padded row"):
        R64.restate(A, B, C0, M, N, Kd, Kd, Kd, N, True, True, row_lens=lens, row_T=T, row_halo=1)
    t = torch.arange(M) % T
    dead = t >= lens.long()[torch.arange(M) // T] + 1
    A[dead] = 0
    out = R64.restate(A, B, C0, M, N, Kd, Kd, Kd, N, True, True, row_lens=lens, row_T=T, row_halo=1)
    _close(out.C.view(M, N), A @ B.t())
    assert bool((out.C.view(M, N)[dead] == 0).all()) and bool(out.written_C.all())
    # TN: the reduction rows in padding must be zero in A (the caller's duty); B may hold anything there
    At, Bt = _r(g, M, 5), _r(g, M, N)
    with pytest.raises(ValueError, match="caller's duty"):
        R64.restate(At, Bt, torch.zeros(5 * N, dtype=D), 5, N, M, 5, N, N, False, False, row_lens=lens, row_T=T, row_halo=1)
    At[dead] = 0
    out = R64.restate(At, Bt, torch.zeros(5 * N, dtype=D), 5, N, M, 5, N, N, False, False, row_lens=lens, row_T=T, row_halo=1)
    _close(out.C.view(5, N), At.t() @ Bt)


# ---- the case table against the route query -----------------------------------------------------------------------------------------

def test_case_ids_are_unique_and_every_kind_has_shape_and_feature_cases():
    ids = [c.id for c in G.CASES]
    assert len(set(ids)) == len(ids)
    for kind in G.KINDS:
        shapes = [c for c in G.CASES if c.kind == kind and c.feature == "shape"]
        assert 4 <= len(shapes) <= 12, (kind, len(shapes))
        assert G.BASE[kind] in [(c.layout, c.M, c.N, c.K) for c in shapes], kind
        assert all(c.recipe == "exact" for c in shapes)
    assert set(G.KINDS) <= set(_lib.GEMM_KINDS)


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_every_table_row_routes_to_the_kind_it_names(case):
    p = G.build(case, contents=False)
    route = G.route_of(p)
    assert route.kind == case.kind, route
    tile = G.SK_RAGGED_TILE if (case.kind == "stream_k" and p.want_map) else G.TILE[case.kind]
    assert (route.tile_m, route.tile_n) == tile and route.k_granule == G.GRANULE[case.kind], route
    assert G.takes(p, case.kind)
    if case.recipe == "exact":          # structural cases compare for equality: nothing a tolerance could hide
        assert case.feature not in G.RANDOM


@pytest.mark.parametrize("kind", G.KINDS)
def test_the_feature_list_of_a_kind_is_exactly_what_its_route_keeps(kind):
    """for every (kind, feature): the pair is in the table if and only if ctts_gemm_route still names the kind at the kind's base shape
    with the feature switched on (a descriptor the library refuses counts as not taken)"""
    layout, M, N, Kd = G.BASE[kind]
    listed = {c.feature for c in G.CASES if c.kind == kind and c.feature != "shape"}
    assert listed == set(G.TAKES[kind])
    for feat in G.FEATURES:
        c = G.Case(f"base-{kind}-{feat}", kind, layout, M, N, Kd, feat, "random" if feat in G.RANDOM else "exact")
        try:
            taken = G.takes(G.build(c, contents=False), kind)
        except _lib.CttsError:
            taken = False
        assert taken == (feat in listed), (kind, feat, taken)
