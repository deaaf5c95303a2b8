"""CPU: kernels.gemm_views derives the ctts_gemm_desc fields of a launch from three tensor views, and the operators of ops.py that describe
their GEMMs that way launch exactly what their hand-written descriptors used to say.  Nothing is launched and the library is not loaded:
the derivation is pure, and the operators run on CPU tensors behind recording stand-ins for the kernel wrappers (as in
test_linear_layer_plan_cpu.py).  Numerics are held by the GPU tests."""
import inspect

import pytest
import torch

import ctts_amd  # noqa: F401
from ctts_amd import kernels as K
from ctts_amd import ops
from ctts_amd._lib import CttsError

B, H, T, dh = 3, 2, 10, 4
C, C2, C3 = H * dh, 2 * H * dh, 3 * H * dh
sP = (H * T * T, T * T)          # batch strides of a [B, H, T, T] map


def addr(t):
    """where a view starts: (its storage, element offset)"""
    return t.untyped_storage().data_ptr(), t.storage_offset()


def heads(x, parts=1):
    """[B, H, T, dh] views of the channel blocks of x [B, T, parts * C]"""
    return x.view(x.shape[0], x.shape[1], parts, H, dh).permute(2, 0, 3, 1, 4).unbind(0)


# ---- 1. the derivation table ----------------------------------------------------------------------------------------------------------
def _table():
    """name -> (A, B, C views, the tensors they start in with element offsets, (M, N, K, lda, ldb, ldc, a_kc, b_kc), keywords)"""
    z = torch.zeros
    a56, a65, b67, w76, c57 = z(5, 6), z(6, 5), z(6, 7), z(7, 6), z(5, 7)
    a3, b3, c3 = z(B, 5, 6), z(B, 6, 7), z(B, 5, 7)
    qkv, dqkv, S, dO, pos, qv = z(B, T, C3), z(B, T, C3), z(B, H, T, T), z(B, T, C), z(T, C), z(B, T, C)
    (q, k, v), (dq, dk, dv), (dOh,), (qvh,) = heads(qkv, 3), heads(dqkv, 3), heads(dO), heads(qv)
    posh = heads(pos.unsqueeze(0))[0].expand(B, H, T, dh)
    ones, g, dvec = torch.ones(B, 1, T), z(B, T, C), z(B, 1, C)
    nd, Hh, rows = 2, 8, 30
    dgh, hp, dw = z(rows, nd * 3 * Hh), z(rows, nd * Hh), z(nd, 3 * Hh, Hh)
    Bm, N, hop, nfft, nre = 2, 4096, 256, 1024, 1026
    F, W = 1 + N // hop, N + nfft
    ypad, basis, reim = z(Bm, W), z(nre, nfft), z(Bm * F, nre)
    one = dict(nb0=1, nb1=1, sA=(0, 0), sB=(0, 0), sC=(0, 0))
    hd = dict(nb0=B, nb1=H)
    return {
        "2d A row-major, B column-major": (a56, w76.t(), c57, ((a56, 0), (w76, 0), (c57, 0)), (5, 7, 6, 6, 6, 7, True, True), one),
        "2d A column-major, B row-major": (a65.t(), b67, c57, ((a65, 0), (b67, 0), (c57, 0)), (5, 7, 6, 5, 7, 7, False, False), one),
        "3d": (a3, b3, c3, ((a3, 0), (b3, 0), (c3, 0)), (5, 7, 6, 6, 7, 7, True, False),
               dict(nb0=B, nb1=1, sA=(30, 0), sB=(42, 0), sC=(35, 0))),
        "4d Q K^T, k at offset C of qkv": (q, k.transpose(-1, -2), S, ((qkv, 0), (qkv, C), (S, 0)), (T, T, dh, C3, C3, T, True, True),
                                           dict(hd, sA=(T * C3, dh), sB=(T * C3, dh), sC=sP)),
        "4d dV = P^T dO into offset 2C of dqkv": (S.transpose(-1, -2), dOh, dv, ((S, 0), (dO, 0), (dqkv, 2 * C)),
                                                  (T, dh, T, T, C, C3, False, False), dict(hd, sA=sP, sB=(T * C, dh), sC=(T * C3, dh))),
        "4d dK = dS^T Q into offset C of dqkv": (S.transpose(-1, -2), q, dk, ((S, 0), (qkv, 0), (dqkv, C)),
                                                 (T, dh, T, T, C3, C3, False, False), dict(hd, sA=sP, sB=(T * C3, dh), sC=(T * C3, dh))),
        "expanded batch level: qv pos^T": (qvh, posh.transpose(-1, -2), S, ((qv, 0), (pos, 0), (S, 0)), (T, T, dh, C, C, T, True, True),
                                           dict(hd, sA=(T * C, dh), sB=(0, dh), sC=sP)),
        "size-1 M: add_over_time": (ones, g, dvec, ((ones, 0), (g, 0), (dvec, 0)), (1, C, T, T, C, C, True, False),
                                    dict(nb0=B, nb1=1, sA=(T, 0), sB=(T * C, 0), sC=(C, 0))),
        "2d column slices: GRU dW_hh[1]": (dgh[:, 3 * Hh:].t(), hp[:, Hh:], dw[1], ((dgh, 3 * Hh), (hp, Hh), (dw, 3 * Hh * Hh)),
                                           (3 * Hh, Hh, rows, nd * 3 * Hh, nd * Hh, Hh, False, False), one),
        "as_strided rows closer than K: mel frames": (ypad.as_strided((Bm, F, nfft), (W, hop, 1)), basis.t().expand(Bm, nfft, nre),
                                                      reim.view(Bm, F, nre), ((ypad, 0), (basis, 0), (reim, 0)),
                                                      (F, nre, nfft, hop, nfft, nre, True, True),
                                                      dict(nb0=Bm, nb1=1, sA=(W, 0), sB=(0, 0), sC=(F * nre, 0))),
    }


@pytest.mark.parametrize("case", list(_table()))
def test_gemm_views_derives_the_descriptor(case):
    A, Bv, Cv, bases, dims, kw = _table()[case]
    args, got_kw = K.gemm_views(A, Bv, Cv)
    assert args[0] is A and args[1] is Bv and args[2] is Cv          # the views themselves: data_ptr() carries the offset
    assert [addr(t) for t in args[:3]] == [(t.untyped_storage().data_ptr(), off) for t, off in bases]
    assert tuple(args[3:]) == dims and all(type(f) is bool for f in args[9:])
    assert got_kw == kw
    inspect.signature(K._gemm_desc).bind(*args, **got_kw)            # the (args, kw) of K.gemm / gemm_route / gemm_takes_*


# ---- 2. what it refuses ---------------------------------------------------------------------------------------------------------------
def _refusals():
    z = torch.zeros
    a, b, c = z(B, 5, 6), z(B, 6, 7), z(B, 5, 7)
    return {
        "A not float32": (lambda: K.gemm_views(a.double(), b, c), "^A:"),
        "B not float32": (lambda: K.gemm_views(a, b.half(), c), "^B:"),
        "C not float32": (lambda: K.gemm_views(a, b, c.to(torch.bfloat16)), "^C:"),
        "three batch dimensions": (lambda: K.gemm_views(z(2, 2, 2, 5, 6), z(2, 2, 2, 6, 7), z(2, 2, 2, 5, 7)), "^C:"),
        "A with more batch dimensions than C": (lambda: K.gemm_views(z(2, B, 5, 6), b, c), "^A:"),
        "batch size of A neither equal nor 1": (lambda: K.gemm_views(z(2, 5, 6), b, c), "^A:"),
        "batch size of B neither equal nor 1": (lambda: K.gemm_views(a, z(B + 1, 6, 7), c), "^B:"),
        "A strided both ways": (lambda: K.gemm_views(z(B, 5, 12)[:, :, ::2], b, c), "^A:"),
        "B strided both ways": (lambda: K.gemm_views(a, z(B, 12, 14)[:, ::2, ::2], c), "^B:"),
        "C with non-unit inner stride": (lambda: K.gemm_views(a, b, z(B, 5, 14)[:, :, ::2]), "^C:"),
        "C column-major": (lambda: K.gemm_views(a, b, z(B, 7, 5).transpose(-1, -2)), "^C:"),
        "C with zero inner stride": (lambda: K.gemm_views(a, b, z(B, 5, 1).expand(B, 5, 7)), "^C:"),
        "K disagrees": (lambda: K.gemm_views(a, z(B, 5, 7), c), "^inner extents"),
        "M disagrees": (lambda: K.gemm_views(a, b, z(B, 4, 7)), "^inner extents"),
        "N disagrees": (lambda: K.gemm_views(a, b, z(B, 5, 8)), "^inner extents"),
        "E with another leading dimension": (lambda: K.gemm_views(a, b, c, E=z(B, 5, 8)[:, :, :7]), "^E:"),
        "E with other batch strides": (lambda: K.gemm_views(a, b, c, E=z(B, 6, 7)[:, :5]), "^E:"),
        "E of another shape": (lambda: K.gemm_views(a, b, c, E=z(B, 5, 6)), "^E:"),
        "E not float32": (lambda: K.gemm_views(a, b, c, E=z(B, 5, 7).double()), "^E:"),
        "lens of another count than nb0": (lambda: K.gemm_views(a, b, c, lens=z(B + 1, dtype=torch.int32)), "^lens:"),
    }


@pytest.mark.parametrize("case", list(_refusals()))
def test_gemm_views_refuses_and_names_the_operand(case):
    call, word = _refusals()[case]
    with pytest.raises(CttsError, match=word):
        call()


def test_gemm_views_accepts_a_matching_epilogue_operand_and_lens():
    a, b, wide = torch.zeros(B, 5, 6), torch.zeros(B, 6, 7), torch.zeros(2, B, 5, 8)
    K.gemm_views(a, b, wide[0, :, :, :7], E=wide[1, :, :, :7], lens=torch.zeros(B, dtype=torch.int32))


def test_bgemm_is_gemm_on_the_derived_description(monkeypatch):
    seen = []
    monkeypatch.setattr(K, "gemm", lambda *args, **kw: seen.append((args, kw)) or args[2])
    P, dO, dqkv, lens = torch.zeros(B, H, T, T), torch.zeros(B, T, C), torch.zeros(B, T, C3), torch.zeros(B, dtype=torch.int32)
    dv = heads(dqkv, 3)[2]
    assert K.bgemm(P.transpose(-1, -2), heads(dO)[0], dv, lens=lens, lim=(1, 0, 1), split_k=2, split_overwrite=True) is dv
    (args, kw), = seen
    assert tuple(args[3:]) == (T, dh, T, T, C, C3, False, False)
    assert kw == dict(nb0=B, nb1=H, sA=sP, sB=(T * C, dh), sC=(T * C3, dh), lens=lens, lim=(1, 0, 1), split_k=2, split_overwrite=True)
    with pytest.raises(CttsError, match="lens"):
        K.bgemm(P.transpose(-1, -2), heads(dO)[0], dv, lens=lens[:2])
    assert len(seen) == 1


# ---- 3. the launch plan of every operator that describes its GEMMs by views --------------------------------------------------------------
# Each expectation below is the K.gemm call of the operator as it was written before the views (positional numbers, element offsets, stride
# pairs), one line per launch in program order: (A, B, C, (M, N, K, lda, ldb, ldc, a_kc, b_kc), keywords that differ from the descriptor's
# defaults).  An operand is a tensor name or (name, element offset into that tensor's storage); names are bound to storages on first
# sight and must then stay put, so two operands share a name exactly when they share memory.
DESC = inspect.signature(K._gemm_desc)


class Recorder:
    """stand-ins for the kernel wrappers: record the gemm calls (keeping their tensors alive), return tensors of the right shape"""

    def __init__(self, monkeypatch):
        self.calls = []
        for name in [n for n in dir(self) if not n.startswith("_") and n != "calls"]:
            monkeypatch.setattr(K, name, getattr(self, name))

    def gemm(self, *args, **kw):
        self.calls.append((args, kw))
        return args[2]

    def softmax_fwd(self, S, lens, nb0, nb1, T_):
        return S

    def rowdot_heads(self, a, b, n_heads):
        return torch.zeros(a.shape[0], n_heads, a.shape[1])

    def relpos_softmax_fwd(self, S, PS, T_, scale, p_drop=0.0, seed=None, drop_offset=0, want_dropped=True):
        return torch.zeros_like(S) if want_dropped else None

    def relpos_softmax_bwd(self, P, dPd, T_, scale, p_drop=0.0, seed=None, drop_offset=0):
        return dPd

    def relshift_bwd(self, dS, T_):
        return torch.zeros_like(dS)

    def rowscale_dropout(self, x, rowscale=None, p_drop=0.0, seed=None, drop_offset=0):
        return torch.zeros_like(x)

    def colsum(self, x2d, ld=None, scale=1.0, acc_into=None):
        return acc_into if acc_into is not None else torch.zeros(x2d.shape[1])

    def neg_sqdist(self, q, k, temp):
        return torch.zeros(q.shape[0], q.shape[1], k.shape[1])

    def gru_fwd(self, gi, whh, bhh, Hh, ndir, save_gates=True, rev_mask=None):
        return torch.zeros(*gi.shape[:2], ndir * Hh), torch.zeros(*gi.shape[:2], ndir * 4 * Hh)

    def gru_bwd(self, dout, out, gates, whh, Hh, ndir, rev_mask=None):
        return torch.zeros(*out.shape[:2], ndir * 3 * Hh), torch.zeros(*out.shape[:2], ndir * 3 * Hh), torch.zeros_like(out)

    def reflect_pad(self, y, pad):
        return torch.zeros(y.shape[0], (y.shape[1] + 2 * pad + 3) // 4 * 4)

    def stft_magnitude(self, reim, frames, nbins, ld_mag):
        return torch.zeros(frames, ld_mag), torch.zeros(frames)

    def log_clamp_transpose(self, mel_fm, B_, F, n_mel, clip):
        return torch.zeros(B_, n_mel, F)

    def fastformer_pool_fwd(self, s, V, lens, B_, T_, H_, div):
        return torch.zeros(B_, V.shape[-1]), torch.zeros(B_, H_, 2)

    def fastformer_pool_bwd(self, dp, p, stats, s, V, lens, B_, T_, H_, div, dV_in=None):
        return (dV_in if dV_in is not None else torch.zeros(B_ * T_, V.shape[-1])), torch.zeros(B_ * T_, H_)

    def fastformer_bcast(self, X, p, B_, T_):
        return torch.zeros(B_ * T_, X.shape[-1])

    def fastformer_bcast_bwd(self, dY1, X, p, B_, T_, dY2=None, dX_in=None, out=None):
        return (out if out is not None else torch.zeros(B_ * T_, X.shape[-1])), torch.zeros(B_, X.shape[-1])


@pytest.fixture
def rec(monkeypatch):
    return Recorder(monkeypatch)


def assert_launches(calls, expected, known):
    """`known`: name -> tensor for the tensors the test itself holds (inputs, results, gradients)"""
    bound = {name: t.untyped_storage().data_ptr() for name, t in known.items()}

    def same_tensor(got, want, what, got_off=0):
        name, off = want if isinstance(want, tuple) else (want, 0)
        st, got_off = got.untyped_storage().data_ptr(), got.storage_offset() + got_off
        if name not in bound:
            assert st not in bound.values(), f"{what}: a new name {name!r} for memory that already has one"
            bound[name] = st
        assert (st, got_off) == (bound[name], off), f"{what}: not {name} + {off}"

    assert len(calls) == len(expected)
    for i, ((args, kw), (eA, eB, eC, dims, ekw)) in enumerate(zip(calls, expected)):
        kw = dict(kw)
        defer = bool(kw.pop("defer", False))
        full = DESC.bind(*args, **kw)
        full.apply_defaults()
        full = dict(full.arguments)
        for key, want in (("A", eA), ("B", eB), ("Cout", eC)):
            same_tensor(full.pop(key), want, f"launch {i} operand {key}", full.pop(key[0].lower() + "_off"))
        got_dims = tuple(int(full.pop(k)) for k in ("M", "N", "K", "lda", "ldb", "ldc")) + tuple(bool(full.pop(k)) for k in ("a_kc", "b_kc"))
        assert got_dims == dims, f"launch {i}: {got_dims} != {dims}"
        assert defer == bool(ekw.get("defer", False)), f"launch {i}: defer"
        for key, got in full.items():
            want = ekw.get(key, DESC.parameters[key].default)
            if torch.is_tensor(got):
                assert isinstance(want, (str, tuple)), f"launch {i}: unexpected tensor for {key}"
                same_tensor(got, want, f"launch {i} {key}")
            elif isinstance(got, (tuple, list)):
                assert tuple(int(v) for v in got) == tuple(want), f"launch {i}: {key} = {got}, expected {want}"
            else:
                assert got == want and not isinstance(want, str), f"launch {i}: {key} = {got!r}, expected {want!r}"
        assert set(ekw) <= set(full) | {"defer"}, f"launch {i}: expectation names unknown keywords"
    for name, t in known.items():
        assert name in bound


def test_self_attention_launches(rec):
    qkv, lens, dO = torch.randn(B, T, C3, requires_grad=True), torch.tensor([T, 7, 3], dtype=torch.int32), torch.randn(B, T, C)
    out = ops._SelfAttention.apply(qkv, lens, H)
    dqkv, = torch.autograd.grad(out, qkv, dO)
    hd = dict(nb0=B, nb1=H, lens="lens")
    wide, scale = dict(hd, lim=(1, 0, 1), split_overwrite=True), dh ** -0.5
    assert_launches(rec.calls, [
        ("qkv", ("qkv", C), "S", (T, T, dh, C3, C3, T, True, True), dict(hd, sA=(T * C3, dh), sB=(T * C3, dh), sC=sP, lim=(1, 1, 0), alpha=scale)),
        ("S", ("qkv", 2 * C), "out", (T, dh, T, T, C3, C, True, False), dict(wide, sA=sP, sB=(T * C3, dh), sC=(T * C, dh))),
        # dV, dP (softmax backward in the epilogue: E = P, rowsub = D), dQ, dK
        ("S", "dO", ("dqkv", 2 * C), (T, dh, T, T, C, C3, False, False), dict(wide, sA=sP, sB=(T * C, dh), sC=(T * C3, dh))),
        ("dO", ("qkv", 2 * C), "dP", (T, T, dh, C, C3, T, True, True),
         dict(hd, sA=(T * C, dh), sB=(T * C3, dh), sC=sP, lim=(1, 1, 0), E="S", rowsub="Dv")),
        ("dP", ("qkv", C), "dqkv", (T, dh, T, T, C3, C3, True, False), dict(wide, sA=sP, sB=(T * C3, dh), sC=(T * C3, dh), alpha=scale)),
        ("dP", "qkv", ("dqkv", C), (T, dh, T, T, C3, C3, False, False), dict(wide, sA=sP, sB=(T * C3, dh), sC=(T * C3, dh), alpha=scale)),
    ], dict(qkv=qkv, lens=lens, out=out, dO=dO, dqkv=dqkv))


def test_relpos_attention_launches(rec):
    qu, qv, kv, pos = (torch.randn(*s, requires_grad=True) for s in ((B, T, C), (B, T, C), (B, T, C2), (T, C)))
    dO, seed = torch.randn(B, T, C), torch.zeros(1, dtype=torch.int64)
    out = ops._RelPosAttention.apply(qu, qv, kv, pos, H, 0.25, 0.1, seed, 5)
    dqu, dqv, dkv, dpos = torch.autograd.grad(out, [qu, qv, kv, pos], dO)
    hd = dict(nb0=B, nb1=H)
    x, kvs, m = (T * C, dh), (T * C2, dh), sP
    assert_launches(rec.calls, [
        ("qu", "kv", "S", (T, T, dh, C, C2, T, True, True), dict(hd, sA=x, sB=kvs, sC=m)),
        ("qv", "pos", "PS", (T, T, dh, C, C, T, True, True), dict(hd, sA=x, sB=(0, dh), sC=m)),
        ("Pd", ("kv", C), "out", (T, dh, T, T, C2, C, True, False), dict(hd, sA=m, sB=kvs, sC=x)),
        # dV (Pd regenerated), dPd, dQU, dK, dQV, dpos per batch
        ("Pd again", "dO", ("dkv", C), (T, dh, T, T, C, C2, False, False), dict(hd, sA=m, sB=x, sC=kvs)),
        ("dO", ("kv", C), "dS", (T, T, dh, C, C2, T, True, True), dict(hd, sA=x, sB=kvs, sC=m)),
        ("dS", "kv", "dqu", (T, dh, T, T, C2, C, True, False), dict(hd, sA=m, sB=kvs, sC=x)),
        ("dS", "qu", "dkv", (T, dh, T, T, C, C2, False, False), dict(hd, sA=m, sB=x, sC=kvs)),
        ("dPS", "pos", "dqv", (T, dh, T, T, C, C, True, False), dict(hd, sA=m, sB=(0, dh), sC=x)),
        ("dPS", "qv", "dpos_b", (T, dh, T, T, C, C, False, False), dict(hd, sA=m, sB=x, sC=x)),
    ], dict(qu=qu, qv=qv, kv=kv, pos=pos, out=out, dO=dO, dqu=dqu, dqv=dqv, dkv=dkv))


M, N, Kd = 5, 7, 6


def test_bmm_nn_launches(rec):
    A, X, dO = torch.randn(B, M, Kd, requires_grad=True), torch.randn(B, Kd, N, requires_grad=True), torch.randn(B, M, N)
    out = ops.bmm_nn(A, X)
    dA, dX = torch.autograd.grad(out, [A, X], dO)
    assert_launches(rec.calls, [
        ("A", "X", "out", (M, N, Kd, Kd, N, N, True, False), dict(nb0=B, sA=(M * Kd, 0), sB=(Kd * N, 0), sC=(M * N, 0))),
        ("dO", "X", "dA", (M, Kd, N, N, N, Kd, True, True), dict(nb0=B, sA=(M * N, 0), sB=(Kd * N, 0), sC=(M * Kd, 0))),
        ("A", "dO", "dX", (Kd, N, M, Kd, N, N, False, False), dict(nb0=B, sA=(M * Kd, 0), sB=(M * N, 0), sC=(Kd * N, 0))),
    ], dict(A=A, X=X, out=out, dO=dO, dA=dA, dX=dX))


def test_bmm_nt_launches(rec):
    A, Bm, dO = torch.randn(B, M, Kd, requires_grad=True), torch.randn(B, N, Kd, requires_grad=True), torch.randn(B, M, N)
    out = ops.bmm_nt(A, Bm, 0.5)
    dA, dB = torch.autograd.grad(out, [A, Bm], dO)
    assert_launches(rec.calls, [
        ("A", "Bm", "out", (M, N, Kd, Kd, Kd, N, True, True), dict(nb0=B, sA=(M * Kd, 0), sB=(N * Kd, 0), sC=(M * N, 0), alpha=0.5)),
        ("dO", "Bm", "dA", (M, Kd, N, N, Kd, Kd, True, False), dict(nb0=B, sA=(M * N, 0), sB=(N * Kd, 0), sC=(M * Kd, 0), alpha=0.5)),
        ("dO", "A", "dB", (N, Kd, M, N, Kd, Kd, False, False), dict(nb0=B, sA=(M * N, 0), sB=(M * Kd, 0), sC=(N * Kd, 0), alpha=0.5)),
    ], dict(A=A, Bm=Bm, out=out, dO=dO, dA=dA, dB=dB))


def test_neg_sqdist_backward_launches(rec):
    Tq, Tk, Cc, C1 = 10, 6, 5, 8          # C1: Cc + the ones column, rounded up to a multiple of four
    q, k, g = torch.randn(B, Tq, Cc, requires_grad=True), torch.randn(B, Tk, Cc, requires_grad=True), torch.randn(B, Tq, Tk)
    torch.autograd.grad(ops.neg_sqdist(q, k, 0.0005), [q, k], g)
    assert_launches(rec.calls, [
        ("g", "k | 1", "g k", (Tq, C1, Tk, Tk, C1, C1, True, False), dict(nb0=B, sA=(Tq * Tk, 0), sB=(Tk * C1, 0), sC=(Tq * C1, 0))),
        ("g", "q | 1", "g^T q", (Tk, C1, Tq, Tk, C1, C1, False, False), dict(nb0=B, sA=(Tq * Tk, 0), sB=(Tq * C1, 0), sC=(Tk * C1, 0))),
    ], dict(g=g))


def test_add_over_time_backward_launch(rec):
    x, v, g = torch.randn(B, T, C), torch.randn(B, 1, C, requires_grad=True), torch.randn(B, T, C)
    dv, = torch.autograd.grad(ops.add_over_time(x, v), v, g)
    assert_launches(rec.calls, [
        ("ones", "g", "dv", (1, C, T, T, C, C, True, False), dict(nb0=B, sA=(T, 0), sB=(T * C, 0), sC=(C, 0))),
    ], dict(g=g, dv=dv))


def test_gru_backward_launches(rec):
    nd, Hh = 2, 8
    rows = B * T
    gi, whh, bhh = (torch.randn(*s, requires_grad=True) for s in ((B, T, nd * 3 * Hh), (nd, 3 * Hh, Hh), (nd, 3 * Hh)))
    out = ops._GRU.apply(gi, whh, bhh, Hh, nd)
    dgi, dwhh, dbhh = torch.autograd.grad(out, [gi, whh, bhh], torch.randn(B, T, nd * Hh))
    assert_launches(rec.calls, [
        (("dgh", d * 3 * Hh), ("hprev", d * Hh), ("dwhh", d * 3 * Hh * Hh), (3 * Hh, Hh, rows, nd * 3 * Hh, nd * Hh, Hh, False, False),
         dict(split_k=2, split_overwrite=True)) for d in range(nd)
    ], dict(dwhh=dwhh))


def _packed(adjacent):
    Kin, sizes = 8, (8, 8, 8)
    if not adjacent:
        return [torch.randn(n, Kin, requires_grad=True) for n in sizes], None
    flat, grads = torch.randn(sum(sizes) * Kin), torch.zeros(sum(sizes) * Kin)
    ws = [c.view(n, Kin).requires_grad_() for c, n in zip(flat.split([n * Kin for n in sizes]), sizes)]
    for w, gslab in zip(ws, grads.split([n * Kin for n in sizes])):
        w.grad = gslab.view_as(w)
    return ws, grads


def test_packed_linear_launches_on_adjacent_weights(rec):
    """the stacked weight and its gradient are views of the flat arenas; the weight gradient is ADDED there (deferred split-K sum)"""
    ws, grads = _packed(True)
    ops.set_grad_accumulation_fusion(True)
    x, dY = torch.randn(B, T, 8, requires_grad=True), torch.randn(B, T, 24)
    out = ops.linear_packed(x, ws)
    dX, *dws = torch.autograd.grad(out, [x] + ws, dY, allow_unused=True)
    assert dws == [None] * 3
    assert_launches(rec.calls, [
        ("x", "w", "out", (B * T, 24, 8, 8, 8, 24, True, True), {}),
        ("dY", "w", "dX", (B * T, 8, 24, 24, 8, 8, True, False), {}),
        ("dY", "x", "grads", (24, 8, B * T, 24, 8, 8, False, False), dict(split_k=2, defer=True)),
    ], dict(x=x, w=ws[0], out=out, dY=dY, dX=dX, grads=grads))


def test_packed_linear_launches_on_separate_weights(rec):
    ws, _ = _packed(False)
    x, dY = torch.randn(B, T, 8, requires_grad=True), torch.randn(B, T, 24)
    out = ops.linear_packed(x, ws)
    dX, *dws = torch.autograd.grad(out, [x] + ws, dY)
    assert_launches(rec.calls, [
        ("x", "cat(w)", "out", (B * T, 24, 8, 8, 8, 24, True, True), {}),
        ("dY", "cat(w) again", "dX", (B * T, 8, 24, 24, 8, 8, True, False), {}),
        ("dY", "x", "dW", (24, 8, B * T, 24, 8, 8, False, False), dict(split_k=2, split_overwrite=True)),
    ], dict(x=x, out=out, dY=dY, dX=dX, dW=dws[0]))


def test_fast_attention_launches(rec):
    Cc, Mr = C, B * T
    h, lens, dout = torch.randn(B, T, Cc, requires_grad=True), torch.tensor([T, 7, 3], dtype=torch.int32), torch.randn(B, T, Cc)
    par = {n: torch.randn(*s, requires_grad=True) for n, s in dict(wq=(Cc, Cc), bq=(Cc,), wk=(Cc, Cc), bk=(Cc,), wql=(H, Cc), bql=(H,),
                                                                    wkl=(H, Cc), bkl=(H,), wt=(Cc, Cc), bt=(Cc,)).items()}
    out = ops.fast_attention(h, lens, H, *par.values())
    grads = torch.autograd.grad(out, [h] + list(par.values()), dout)
    sq, lin, low = (Mr, Cc, Cc, Cc, Cc, Cc, True, True), (Mr, H, Cc, Cc, Cc, H, True, True), (Mr, Cc, H, H, Cc, Cc, True, False)
    dsq, wg = (Mr, Cc, Cc, Cc, Cc, Cc, True, False), dict(split_k=2, split_overwrite=True)
    assert_launches(rec.calls, [
        ("h", "wq", "Q", sq, dict(bias="bq", ldr=Cc)),
        ("h", "wk", "K", sq, dict(bias="bk", ldr=Cc)),
        ("Q", "wql", "s_q", lin, dict(bias="bql", ldr=H)),
        ("QK", "wkl", "s_k", lin, dict(bias="bkl", ldr=H)),
        ("WV", "wt", "out", sq, dict(bias="bt", R="Q", ldr=Cc)),
        # backward: data gradients through _ff_dgrad (the residual gradient rides in R), weight gradients through ops._matmul_wgrad
        ("dout", "wt", "dWV", dsq, dict(ldr=Cc)),
        ("dout", "WV", "dwt", (Cc, Cc, Mr, Cc, Cc, Cc, False, False), wg),
        ("ds_k", "wkl", "dQK", low, dict(ldr=Cc)),
        ("ds_k", "QK", "dwkl", (H, Cc, Mr, H, Cc, Cc, False, False), wg),
        ("ds_q", "wql", "dQ", low, dict(R="dQ so far", ldr=Cc)),
        ("ds_q", "Q", "dwql", (H, Cc, Mr, H, Cc, Cc, False, False), wg),
        ("dK", "wk", "dh of K", dsq, dict(ldr=Cc)),
        ("dQ", "wq", "dh", dsq, dict(R="dh of K", ldr=Cc)),
        ("dQ", "h", "dwq", (Cc, Cc, Mr, Cc, Cc, Cc, False, False), wg),
        ("dK", "h", "dwk", (Cc, Cc, Mr, Cc, Cc, Cc, False, False), wg),
    ], dict(h=h, out=out, dout=dout, dh=grads[0], **par, **{"d" + n: g for n, g in zip(par, grads[1:]) if n.startswith("w")}))


def test_mel_spectrogram_launches(rec):
    Bm, Nn, hop, n_fft, n_mel, nbins, nre, ld_mag = 2, 4096, 256, 1024, 80, 513, 1026, 516
    F, W = 1 + Nn // hop, Nn + n_fft
    y, basis, melb = torch.randn(Bm, Nn), torch.randn(nre, n_fft), torch.randn(n_mel, ld_mag)
    mel, energy, mag = ops.mel_spectrogram(y, basis, melb, n_fft, hop, n_mel, nbins)
    assert_launches(rec.calls, [
        # frames as overlapping rows of the padded waveform: row stride hop < K = n_fft, one basis for the whole batch
        ("ypad", "basis", "reim", (F, nre, n_fft, hop, n_fft, nre, True, True), dict(nb0=Bm, sA=(W, 0), sC=(F * nre, 0))),
        ("mag", "melb", "mel_fm", (Bm * F, n_mel, ld_mag, ld_mag, ld_mag, n_mel, True, True), {}),
    ], dict(basis=basis, melb=melb, mag=mag))
