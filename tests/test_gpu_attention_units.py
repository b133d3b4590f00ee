"""The attention half's two launches, each alone behind its C-ABI unit wrapper (vb_attention / vb_attention_lens, vb_qkv_rope), against the
float64 row oracles of tests/attn_oracles.py and their derived per-element bounds, at the edges the kernels have: one query row, a key
count that is a multiple of 64 (no partial tile), a last tile of one key, a second workgroup of one row, a wave with one live row, nine
(batch, head) pairs, a cross pass of exactly one tile, a row length of 1, workgroups of padding rows alone.  Every input is followed by
NaN guard elements, every output is pre-filled with a sentinel bit pattern (inside: must be overwritten; behind the end: must come back
bit for bit), V^T pad columns and everything past a row's length hold large finite values (the documented contract says finite: a key
that leaks is then thousands of times the bound).  Each case prints its worst err / bound (pytest -s)."""
import pytest
import torch

from tests import attn_oracles as A
from versband_amd import _lib as L
from versband_amd import pack

pytestmark = pytest.mark.gpu
GUARD = 4096          # guard elements behind every buffer
SENT = 0x7FA5         # sentinel bits of the bf16 outputs (a NaN no kernel writes)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return L.load()


def guarded(t):
    """device copy of t with GUARD NaN elements behind it in the same allocation -> the data as a view at the allocation's start"""
    flat = torch.full((t.numel() + GUARD,), float("nan"), dtype=t.dtype)
    flat[:t.numel()] = t.reshape(-1)
    return flat.cuda()[:t.numel()].view(t.shape)


def sentinel(shape):
    """bf16 output of `shape` pre-filled with SENT, GUARD more sentinels behind it -> (view, the whole buffer as int16)"""
    n = int(torch.tensor(shape).prod())
    buf = torch.full((n + GUARD,), SENT, dtype=torch.int16, device="cuda")
    return buf[:n].view(torch.bfloat16).view(shape), buf


def bits(t):
    return t.contiguous().view(torch.int16)


def guard_intact(buf, n):
    return bool((buf[n:] == SENT).all())


def value(planes):
    """[np][...] bf16 planes -> float64 hi + lo"""
    return planes.double().sum(0)


def vt_planes(x, Spad, np_):
    """[B][S][H][hd] fp32 -> V^T planes [np][B][H][hd][Spad], the pad columns BIG in every plane"""
    B, S, H, hd = x.shape
    o = torch.full((np_, B, H, hd, Spad), A.BIG, dtype=torch.bfloat16)
    o[..., :S] = pack.to_planes(x.permute(0, 2, 3, 1).contiguous(), np_)
    return o


def run_attention(lib, c, np_, use_self, use_cross):
    B, T, H, Lc, lens = c["B"], c["T"], c["H"], c["Lc"], c["lens"]
    Tpad, Lpad = (T + 63) // 64 * 64, (Lc + 63) // 64 * 64
    d = {n: guarded(pack.to_planes(c[n], np_)) for n in ("q", "k", "ky")}
    d["vt"], d["vyt"] = guarded(vt_planes(c["v"], Tpad, np_)), guarded(vt_planes(c["vy"], Lpad, np_))
    cw = guarded(c["cw"])
    out, obuf = sentinel((np_, B, T, H, A.HD))
    args = [L.ptr(d["q"]), L.ptr(d["k"]) if use_self else None, L.ptr(d["vt"]) if use_self else None, L.ptr(d["ky"]) if use_cross else None,
            L.ptr(d["vyt"]) if use_cross else None, L.ptr(cw) if use_cross else None, B, T, Tpad, Lc, Lpad, H, A.HD, np_]
    if lens is not None:
        ld = torch.tensor(lens, dtype=torch.int32, device="cuda")
        L.check(lib.vb_attention_lens(*args, L.ptr(ld), L.ptr(out), L.stream_ptr()), "attention_lens")
    else:
        L.check(lib.vb_attention(*args, L.ptr(out), L.stream_ptr()), "attention")
    torch.cuda.synchronize()
    assert guard_intact(obuf, out.numel()), "attention wrote past the end of its output"
    return out.cpu()


def check_attention(what, c, np_, use_self, use_cross, out):
    """every defined element overwritten and inside the bound; -> worst err / bound"""
    case = (c["B"], c["H"], c["T"], c["Lc"])
    ref, bound = A.attn_reference(*case, c["lens"], np_, use_self, use_cross)
    ok = ~torch.isnan(ref)
    assert not bool((bits(out) == SENT).permute(1, 2, 3, 4, 0).any(-1)[ok].any()), f"{what}: an element of a defined row was never written"
    got = value(out)
    assert bool(torch.isfinite(got).all()), f"{what}: a non-finite output (a guard value read, or an undefined row left unwritten)"
    err = torch.where(ok, (got - ref).abs(), torch.zeros_like(ref))
    bnd = torch.where(ok, bound, torch.ones_like(bound))
    ratio = A.worst(err, bnd)
    print(f"{what}: worst err / bound = {ratio:.3f}")
    if not bool((err <= bnd).all()):
        idx = tuple(int(i) for i in torch.unravel_index((err / bnd).argmax(), err.shape))
        pv = {n: A.plane_values(c[n], np_) for n in ("q", "k", "v", "ky", "vy")}
        dom = A.dominant_pass(pv["q"], pv["k"] if use_self else None, pv["v"] if use_self else None, pv["ky"] if use_cross else None,
                              pv["vy"] if use_cross else None, c["cw"], idx, np_) if c["lens"] is None else "self + cross"
        raise AssertionError(f"{what}: {int((err > bnd).sum())} of {int(ok.sum())} elements outside the bound; worst at (b, t, h, d) = {idx}: "
                             f"error {float(err[idx]):.4e}, bound {float(bnd[idx]):.4e}, reference {float(ref[idx]):.4e} ({dom} dominates)")
    return ratio


# ------------------------------------------------------------------------------------------------------------------ plain attention
@pytest.mark.parametrize("np_", [1, 2])
@pytest.mark.parametrize("B,H,T,Lc", A.PLAIN_CASES)
def test_attention_matches_float64_row_by_row(lib, B, H, T, Lc, np_):
    """(1,1,1,1): one query, one key in either pass.  (1,2,33,64): one wave with one live row, two with none; a cross pass of exactly one
    full tile.  (1,1,64,65): no partial self tile; a cross tile holding one key.  (2,2,65,80): a last self tile of one key.  (1,1,128,1):
    two full tiles, one cross key.  (3,3,129,16): nine (batch, head) pairs - a second group of eight with seven empty slots - and a second
    workgroup of one row.  (1,8,129,65): exactly eight pairs.  Cross only, self only, both."""
    c = A.attn_case(B, H, T, Lc)
    for use_self, use_cross in A.MODES:
        out = run_attention(lib, c, np_, use_self, use_cross)
        check_attention(f"attention {(B, H, T, Lc)} np={np_} self={use_self} cross={use_cross}", c, np_, use_self, use_cross, out)


@pytest.mark.parametrize("np_", [1, 2])
def test_attention_deferred_rescale_keeps_the_bound(lib, np_):
    """VB_ATTN_DEFER = 0 (exact running maximum) and the default 2^8 lie inside the SAME bound (the planted keys of tiles 1 and 2 outgrow
    the first tile's maximum: the rare branch runs); 1e9 - never again after the first tile - is finite, not accurate."""
    c = A.attn_case(*A.DEFER_CASE)
    try:
        for thr in ("0", None, "1e9"):
            L.set_tuning(VB_ATTN_DEFER=thr)
            out = run_attention(lib, c, np_, True, True)
            if thr == "1e9":
                assert bool(torch.isfinite(value(out)).all()), "VB_ATTN_DEFER=1e9: not finite"
            else:
                check_attention(f"attention {A.DEFER_CASE} np={np_} VB_ATTN_DEFER={thr}", c, np_, True, True, out)
    finally:
        L.set_tuning(VB_ATTN_DEFER=None)
        lib.vb_tune_reload()


# ------------------------------------------------------------------------------------------------------------------ row lengths
@pytest.mark.parametrize("np_", [1, 2])
def test_attention_lens_rows_match_float64_on_their_own_keys(lib, np_):
    """T = 130, lens = 130, 129, 128, 65, 64, 1: rows < lens[b] inside the bound of the oracle on that row's own keys (everything past the
    length is large and finite: a leaked key or query shows), rows >= lens[b] finite, and the rows of a workgroup that holds padding
    alone - row 128 on where lens[b] <= 128 - exactly zero in every plane."""
    c = A.attn_case(len(A.LENS), A.LENS_H, A.LENS_T, A.LENS_LC, A.LENS)
    out = run_attention(lib, c, np_, True, True)
    check_attention(f"attention_lens T={A.LENS_T} lens={A.LENS} np={np_}", c, np_, True, True, out)
    for b, n in enumerate(A.LENS):
        if n <= 128:
            assert bool((bits(out)[:, b, 128:] == 0).all()), f"row {b} (len {n}): the padding workgroup's rows are not zero in every plane"


# ------------------------------------------------------------------------------------------------------------------ QKV + RoPE
def qkv_buffers(c, Tpad, np_, zero_vt=False):
    B, T, H = c["B"], c["T"], c["H"]
    D = H * A.HD
    ins = [guarded(pack.to_planes(c["u"], np_)), guarded(pack.to_planes(c["w"], np_)), guarded(c["cos"][:T].contiguous()), guarded(c["sin"][:T].contiguous())]
    q, qb = sentinel((np_, B * T, D))
    k, kb = sentinel((np_, B * T, D))
    vt, vb = sentinel((np_, B, H, A.HD, Tpad))
    if zero_vt:
        vt.zero_()
    return ins, (q, k, vt), (qb, kb, vb)


def run_qkv(lib, c, Tpad, np_, zero_vt=False):
    B, T, H = c["B"], c["T"], c["H"]
    ins, outs, bufs = qkv_buffers(c, Tpad, np_, zero_vt)
    L.check(lib.vb_qkv_rope(*[L.ptr(t) for t in ins], B, T, Tpad, H, A.HD, np_, *[L.ptr(t) for t in outs], L.stream_ptr()), "qkv_rope")
    torch.cuda.synchronize()
    for name, t, buf in zip(("q", "k", "vt"), outs, bufs):
        assert guard_intact(buf, t.numel()), f"qkv_rope wrote past the end of {name}"
    return outs


def check_qkv(what, c, np_, outs):
    B, T = c["B"], c["T"]
    q, k, vt = (t.cpu() for t in outs)
    ref = A.qkv_reference(B, T, np_, c["H"])
    assert bool((bits(vt)[..., T:] == SENT).all()), f"{what}: a V^T pad column >= T was written"
    worst = 0.0
    for name, got, r, bd in zip(("q", "k", "vt"), (q, k, vt[..., :T]), ref[:3], ref[3:]):
        assert not bool((bits(got) == SENT).any()), f"{what}: an element of {name} was never written"
        err = (value(got) - r).abs()
        ratio = A.worst(err, bd)
        print(f"{what} {name}: worst err / bound = {ratio:.3f}")
        assert bool((err <= bd).all()), (f"{what}: {int((err > bd).sum())} of {err.numel()} elements of {name} outside the bound (worst ratio {ratio:.3f} at "
                                         f"{tuple(int(i) for i in torch.unravel_index((err / bd).argmax(), err.shape))})")
        worst = max(worst, ratio)
    return worst


def same_bits(what, a, b):
    for name, x, y in zip(("q", "k", "vt"), a, b):
        bad = (bits(x) != bits(y)).nonzero()
        assert not bad.numel(), f"{what}: {name} differs in {bad.shape[0]} elements, first at {bad[0].tolist()}"


QKV_ROUTES = [dict(VB_QKV_P16_OFF="1"), dict(VB_QKV_VT16_OFF="1"), dict(VB_GEMM_TILE="22"), dict(VB_GEMM_TILE="11"), dict(VB_GEMM_TILE="21"),
              dict(VB_GEMM_TILE="22", VB_QKV_P16_OFF="1"), dict(VB_GEMM_TILE="22", VB_QKV_VT16_OFF="1")]


@pytest.mark.parametrize("np_", [1, 2])
@pytest.mark.parametrize("B,T,Tpad", A.QKV_CASES)
def test_qkv_rope_matches_float64_on_every_route(lib, B, T, Tpad, np_):
    """H = 2 (D = K = 192, N = 576: 4.5 column tiles of 128).  T = 65 / 129: m = b T is a multiple of a T that is no power of two - the
    float-reciprocal decomposition m -> (clip, t) at its edge; T = 64 takes the 16-byte V^T stores on the 128 x 128 route; T = 1: one row.
    q, k and V^T columns < T inside the bound, V^T columns [T, Tpad) and the guards untouched, and every route - the quad epilogue
    (VB_QKV_P16_OFF on 128 x 128 tiles), the P16 epilogue without the 16-byte V^T stores, 128 x 128, 64 x 64, 128 x 64 tiles - gives the
    default route's bits (the launcher's own choice at these sizes: 64 x 64 tiles, LDS-staged epilogue)."""
    c = A.qkv_case(B, T)
    base = run_qkv(lib, c, Tpad, np_)
    check_qkv(f"qkv_rope B={B} T={T} Tpad={Tpad} np={np_}", c, np_, base)
    for knobs in QKV_ROUTES:
        try:
            L.set_tuning(**knobs)
            other = run_qkv(lib, c, Tpad, np_)
        finally:
            L.set_tuning(**{k: None for k in knobs})
        same_bits(f"qkv_rope B={B} T={T} np={np_} under {knobs} vs the default route", other, base)


@pytest.mark.parametrize("np_", [1, 2])
def test_qkv_rope_on_the_8_wave_kernel(lib, np_):
    """the smallest batch of T = 130 clips whose launch makes P8_MIN_TILES 256 x 256 tiles (62 clips, 8060 rows, 2.25 column tiles): the
    8-wave kernel's P16 epilogue against the oracle, and bit for bit against the 4-wave kernels (VB_GEMM_P8_OFF=1)"""
    B, T, Tpad = A.p8_min_clips(), A.QKV_P8_T, 192
    c = A.qkv_case(B, T)
    base = run_qkv(lib, c, Tpad, np_)
    check_qkv(f"qkv_rope B={B} T={T} Tpad={Tpad} np={np_} (8-wave kernel)", c, np_, base)
    try:
        L.set_tuning(VB_GEMM_P8_OFF="1")
        other = run_qkv(lib, c, Tpad, np_)
    finally:
        L.set_tuning(VB_GEMM_P8_OFF=None)
    same_bits(f"qkv_rope B={B} T={T} np={np_} VB_GEMM_P8_OFF=1 vs the 8-wave kernel", other, base)


# ------------------------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("np_", [1, 2])
def test_attention_reads_what_qkv_rope_writes(lib, np_):
    """B, H, T = 2, 2, 65, Tpad = 128, V^T cleared: vb_qkv_rope, then vb_attention (no cross pass) on its q, k and V^T, against the attention
    oracle evaluated on the device's own q, k, V^T read back - the layout contract between the two kernels (pitch Tpad, head-major, d-major)
    independently of either oracle's tolerance for the other stage"""
    B, H, T, Tpad = 2, 2, 65, 128
    c = A.qkv_case(B, T, H)
    q, k, vt = run_qkv(lib, c, Tpad, np_, zero_vt=True)
    out, obuf = sentinel((np_, B, T, H, A.HD))
    L.check(lib.vb_attention(L.ptr(q), L.ptr(k), L.ptr(vt), None, None, None, B, T, Tpad, 1, 64, H, A.HD, np_, L.ptr(out), L.stream_ptr()), "attention")
    torch.cuda.synchronize()
    assert guard_intact(obuf, out.numel()) and not bool((bits(out) == SENT).any())
    qv, kv = (value(t.cpu()).view(B, T, H, A.HD) for t in (q, k))
    vv = value(vt.cpu())[..., :T].permute(0, 3, 1, 2).contiguous()
    assert bool((value(vt.cpu())[..., T:] == 0).all())
    ref, bound = A.attention(qv, kv, vv, None, None, None, None, np_)
    err = (value(out.cpu()) - ref).abs()
    print(f"qkv_rope -> attention np={np_}: worst err / bound = {A.worst(err, bound):.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} elements outside the bound (worst ratio {A.worst(err, bound):.3f})"


def test_qkv_rope_refuses_null_pointers_and_bad_sizes(lib):
    one = torch.zeros(64, device="cuda")
    p, s = L.ptr(one), L.stream_ptr()
    assert lib.vb_qkv_rope(None, p, p, p, 1, 1, 64, 2, 96, 1, p, p, p, s) == -1
    assert lib.vb_qkv_rope(p, p, p, p, 1, 1, 64, 2, 96, 1, p, p, None, s) == -1
    assert lib.vb_qkv_rope(p, p, p, p, 0, 1, 64, 2, 96, 1, p, p, p, s) == -1
    assert lib.vb_qkv_rope(p, p, p, p, 1, 65, 64, 2, 96, 1, p, p, p, s) == -1 and b"qkv_rope" in lib.vb_last_error()
    assert lib.vb_qkv_rope(p, p, p, p, 1, 1, 64, 2, 96, 3, p, p, p, s) == -1
    torch.cuda.synchronize()
