"""GPU: results depend on live rows only, and nothing outside a declared output is written.

Every kernel here works on a live prefix of a larger buffer.  Each case runs an entry point on identical live data, strides
and capacities with every byte OUTSIDE the live region set to zero, then to poison (helpers.dead_values: NaN; huge finite
values of alternating sign, which a running maximum taken with fmaxf would keep where it drops NaN; for the packed INT4
pools nibble bytes 0xFF with scale / zero NaN, +Inf, 65504):

  A. all outputs, and the live rows of pools written in place, are BIT-identical between the runs — no tolerance; the zero
     run is also held to the kernel's existing bar against the oracle, so two runs that agree cannot both be wrong;
  B. outputs and in-place buffers are views into larger buffers (>= 130 guard rows before and after, gap heads either side, a
     gap after every token where the ABI takes a stride): after the call every byte outside the view holds what it held.

Every buffer is allocated at its full declared capacity with >= 130 rows of slack behind the live rows (more than the largest
K tile), so a kernel that ignored its clamp would still read inside the allocation.
"""
import functools

import numpy as np
import pytest
import torch

from helpers import (DEAD_KINDS, INT4_DEAD_KINDS, PARITY_LOG, DeadBuf, _bits, attn_close, dead_embed, dead_values, guard_embed,
                     guard_flat, with_rounded)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
SCALE = D ** -0.5


def _hip():
    from duo_attn import _hip

    _hip.load_library()
    return _hip


def _rand(shape, gen, dtype=torch.bfloat16):
    return torch.randn(shape, generator=gen).to(dtype)


def _snap(*tensors):
    torch.cuda.synchronize()
    return [_bits(t).cpu().clone() for t in tensors]


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape
        n = int((x != y).sum())
        assert n == 0, f"{what}: result {i} differs from the zero-filled run in {n} of {x.numel()} elements"


class _Flags:
    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        _hip().set_debug_flags(self.flags)

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        _hip().set_debug_flags(0)
        return False


def _row2d(live, tail=3, gap=1):
    """[rows, n] (CPU) -> DeadBuf whose rows are 2 * gap + 1 rows' worth of elements apart, `tail` more rows behind"""
    return dead_embed(live[:, None, :], lead=1, tail=tail, gap=gap, device=DEV)


# ============================================================================= 1. bf16 decode
@functools.lru_cache(maxsize=None)
def _bf16_case(group, nf, ns, S, lenF, lenS, seed):
    """live data (CPU) of one attention call + the oracle's answer: q [S, Hq, D], new rows [S, nkv, D], pools or None"""
    from oracle.duo_oracle import flash_attn_func_ref

    g = torch.Generator().manual_seed(seed)
    nkv, Hq = nf + ns, (nf + ns) * group
    q, kn, vn = _rand((S, Hq, D), g), _rand((S, nkv, D), g), _rand((S, nkv, D), g)
    pools = []
    ref, bud, rnd = (torch.empty(S, Hq, D) for _ in range(3))
    for lo, n_h, L in ((0, nf, lenF), (nf, ns, lenS)):
        pk, pv = (_rand((L, n_h, D), g), _rand((L, n_h, D), g)) if L else (None, None)
        pools.append((pk, pv))
        if n_h == 0:
            continue
        kk = torch.cat([pk, kn[:, lo:lo + n_h]]) if L else kn[:, lo:lo + n_h]
        vv = torch.cat([pv, vn[:, lo:lo + n_h]]) if L else vn[:, lo:lo + n_h]
        sl = slice(lo * group, (lo + n_h) * group)
        r, b = flash_attn_func_ref(q[None, :, sl], kk[None], vv[None], round_p=False, out_dtype=torch.float32, return_budget=True)
        ref[:, sl], bud[:, sl] = r[0], b[0]
        if S > 1:
            rnd[:, sl] = flash_attn_func_ref(q[None, :, sl], kk[None], vv[None], round_p=True, out_dtype=torch.bfloat16)[0]
    if S == 1:
        return q, kn, vn, pools, ref, None
    # attn_close's comparison with the reference arithmetic's own noise (with_rounded) holds the kernel to 1.12 x that noise.
    # The figure was measured on launches whose rows see many keys.  The rounded oracle rounds P relative to the row's true
    # maximum, so a row's largest weight is exactly 1.0 and carries no rounding error; the kernel (FA2 too) rounds it like
    # every other weight.  For a row that sees two keys that is one rounding draw against two — a ratio of up to sqrt(2) —
    # and each draw is shared by the row's 128 output elements, so a launch of a few short rows is a few dozen draws, not
    # n elements (measured, zero-filled runs: 1.24 on the first chunk at S = 2, 1.16 at S = 65).  The ratio is therefore
    # asserted where every row sees at least 64 keys (both pools >= 63 rows) and the launch has >= 65 rows per head; the
    # elementwise budget and the absolute rms bar of attn_close hold everywhere, and the measured ratio of the launches left
    # out goes to the parity report ("dead rows: ...") with the kernel flags, forced split and pool layout it was measured under.
    many_keys = S >= 64 and all(L >= 63 for n_h, L in ((nf, lenF), (ns, lenS)) if n_h)
    if not many_keys:
        bud.rounded_ungated = rnd       # recorded, not asserted (_run_bf16_attention)
    return q, kn, vn, pools, ref, (with_rounded(bud, rnd) if many_keys else bud)


def _run_bf16_attention(call, group, nf, ns, S, lenF, lenS, head_major, what, seed=0):
    """``call(q, out, full, stream)`` with q / out [S, Hq, D] views and class descriptors built from views of poisoned pools"""
    h = _hip()
    q, kn, vn, pools, ref, bud = _bf16_case(group, nf, ns, S, lenF, lenS, seed)
    qb = dead_embed(q, lead=2, device=DEV)
    kb, vb = dead_embed(kn, lead=2, device=DEV), dead_embed(vn, lead=2, device=DEV)
    pb = [[dead_embed(t, cap=t.shape[0] + 130, head_major=head_major, device=DEV) if t is not None else None for t in p] for p in pools]
    ob = guard_embed((S, (nf + ns) * group, D), torch.bfloat16, device=DEV)
    bufs = [qb, kb, vb] + [t for p in pb for t in p if t is not None]
    zero = None
    for kind in ("zero",) + DEAD_KINDS:
        for b in bufs:
            b.reset(kind)
        ob.reset("guard")
        cls = []
        for (lo, n_h), (pk, pv) in zip(((0, nf), (nf, ns)), pb):
            segA = h.make_seg(pk.live, pv.live) if pk is not None else h.make_seg(None, None)
            segB = h.make_seg(kb.view[:, lo:lo + n_h], vb.view[:, lo:lo + n_h])
            cls.append(h.make_class(n_h, lo * group, segA, segB) if n_h else None)
        call(qb.view, ob.view, cls[0], cls[1])
        got = _snap(ob.view)
        ob.assert_dead("guard", what=f"{what} out ({kind})")
        for b in bufs:
            b.assert_dead(kind, what=f"{what} inputs ({kind})")
        if zero is None:
            zero = got
            attn_close(ob.view, ref, "", bud)
            rnd = getattr(bud, "rounded_ungated", None)
            if rnd is not None:     # the ratio attn_close would have asserted, on record (parity report) with flags and layout
                o, noise = ob.view.float().cpu(), (rnd.float() - ref).pow(2).mean().sqrt()
                PARITY_LOG[f"dead rows: {what} hm={head_major} flags={h.load_library().duo_get_debug_flags():#x}"] = {
                    "n": int(o.numel()), "rms_err_over_reference_arithmetic": float((o - ref).pow(2).mean().sqrt() / noise),
                    "asserted": False}
        else:
            _same(got, zero, f"{what} ({kind})")


DECODE_LENS = [1, 63, 64, 65, 257, 5000]


@pytest.mark.parametrize("flags", [0, 512], ids=["scan", "wide"])
@pytest.mark.parametrize("group", [4, 1, 3])
@pytest.mark.parametrize("head_major", [True, False])
def test_bf16_decode(head_major, group, flags):
    """attn_decode over both head classes; 5000 rows are split over workgroups; debug bit 9 = the scan kernel's wide-argument form"""
    h = _hip()
    with _Flags(flags):
        for L in DECODE_LENS:
            _run_bf16_attention(lambda q, out, f, s: h.attn_decode(q[0], out[0], group, f, s, SCALE), group, 2, 1, 1, L,
                                min(L, 1 + L % 50), head_major, f"decode g{group} len {L}", seed=L)


def _run_bf16_batched(S, lenF, lenS, what):
    """attention_batched, B = 2: pools, q, new rows and out with slack rows between the batch rows"""
    h = _hip()
    group, nf, ns, B = 4, 2, 1, 2
    cases = [_bf16_case(group, nf, ns, S, lenF, lenS, 900 + b) for b in range(B)]
    stack = lambda i: torch.stack([c[i] for c in cases])
    qb, kb, vb = (dead_embed(stack(i), lead=2, device=DEV) for i in range(3))
    pb = [[dead_embed(torch.stack([c[3][ci][j] for c in cases]), cap=L + 130, head_major=True, device=DEV) for j in range(2)]
          for ci, L in ((0, lenF), (1, lenS))]
    ob = guard_embed((B, S, (nf + ns) * group, D), torch.bfloat16, device=DEV)
    bufs = [qb, kb, vb] + [t for p in pb for t in p]
    zero = None
    for kind in ("zero",) + DEAD_KINDS:
        for b in bufs:
            b.reset(kind)
        ob.reset("guard")
        cls = [h.make_class(n_h, lo * group, h.make_seg(p[0].live, p[1].live),
                            h.make_seg(kb.view[:, :, lo:lo + n_h], vb.view[:, :, lo:lo + n_h]))
               for (lo, n_h), p in zip(((0, nf), (nf, ns)), pb)]
        h.attention_batched(qb.view, ob.view, group, cls[0], cls[1], SCALE)
        got = _snap(ob.view)
        ob.assert_dead("guard", what=f"{what} out ({kind})")
        if zero is None:
            zero = got
            for b in range(B):
                attn_close(ob.view[b], cases[b][4], "", cases[b][5])
        else:
            _same(got, zero, f"{what} ({kind})")


def test_bf16_decode_batched():
    _run_bf16_batched(1, 300, 20, "batched decode")


# ============================================================================= 2. fused decode layer
FUSED_CASES = {
    # nf, ns, full_len, str_len, plan_full_len (decode_layer_dev only)
    "A-stream-below-window": (2, 2, 300, 5, None),
    "B-stream-full-sliding": (2, 2, 300, 12, None),
    "C-empty-retrieval-pool": (2, 2, 0, 7, None),
    "D-planned-above-device-length": (2, 2, 300, 12, 700),
}


@pytest.mark.parametrize("two_launch", [False, True])
@pytest.mark.parametrize("case", list(FUSED_CASES))
def test_fused_decode_layer(case, two_launch):
    """decode_layer (one and two launches) and, case D, decode_layer_dev with the planned length on a bucket above the
    device-side one (rows [len, plan_len) are poison like every row behind the live ones).  Afterwards pool rows below the
    new live length equal the zero run, rows at or above it still hold the poison bit for bit."""
    from oracle.duo_oracle import OracleBackend, flash_attn_func_ref, rope_ref

    h = _hip()
    nf, ns, full_len, str_len, plan = FUSED_CASES[case]
    group, sink, recent, theta = 4, 4, 8, 5e5
    W, nkv, Hq, pos = sink + recent, nf + ns, (nf + ns) * group, full_len
    g = torch.Generator().manual_seed(full_len + str_len)
    q, k, v = _rand((1, Hq, D), g), _rand((1, nkv, D), g), _rand((1, nkv, D), g)
    fk, fv = _rand((full_len, nf, D), g), _rand((full_len, nf, D), g)
    sk, sv = _rand((str_len, ns, D), g), _rand((str_len, ns, D), g)
    cap = (plan or full_len) + 1 + 130
    fkb, fvb = (dead_embed(t, cap=cap, head_major=True, device=DEV) for t in (fk, fv))
    skb, svb = (dead_embed(t, cap=W, head_major=True, device=DEV) for t in (sk, sv))
    qb, kb, vb = (dead_embed(t, lead=2, device=DEV) for t in (q, k, v))
    ob = guard_embed((1, Hq, D), torch.bfloat16, device=DEV)
    pools, n_new = (fkb, fvb, skb, svb), min(str_len + 1, W)
    zero = None
    for kind in ("zero",) + DEAD_KINDS:
        for b in pools + (qb, kb, vb):
            b.reset(kind)
        ob.reset("guard")
        args = (qb.view[0], kb.view[0], vb.view[0], ob.view[0], nf, fkb.view, fvb.view)
        if plan is None:
            n = h.decode_layer(*args, full_len, skb.view, svb.view, str_len, sink, recent, pos, 1.0, theta, SCALE, two_launch=two_launch)
            assert n == n_new
        else:
            st = torch.tensor([full_len, str_len, pos, 0], dtype=torch.int32, device=DEV)
            h.decode_layer_dev(*args, plan, skb.view, svb.view, str_len, sink, recent, pos, 1.0, theta, SCALE, st, two_launch=two_launch)
        live = [fkb.view[:full_len + 1], fvb.view[:full_len + 1], skb.view[:n_new], svb.view[:n_new]]
        got = _snap(ob.view, *live)
        assert int(h.decode_tickets(torch.device(DEV)).abs().sum()) == 0
        ob.assert_dead("guard", what=f"{case} out ({kind})")
        for b, lv in zip(pools, live):
            b.assert_dead(kind, live=lv, what=f"{case} pool rows at or above the new live length ({kind})")
        for b in (qb, kb, vb):      # the step's inputs are read-only, gaps and live rows alike
            b.assert_dead(kind, what=f"{case} inputs ({kind})")
            assert torch.equal(_bits(b.live), _bits(b.at_live(b.initial)))
        if zero is not None:
            _same(got, zero, f"{case} ({kind})")
            continue
        zero = got
        # the zero run against the oracle, as test_decode_layer_fused has it
        qr, kr = rope_ref(q, pos, 1.0, theta)[0], rope_ref(k, pos, 1.0, theta)[0]
        kw = dict(round_p=False, out_dtype=torch.float32)
        ref = torch.empty(Hq, D)
        kk, vv = torch.cat([fk, kr[None, :nf]]), torch.cat([fv, v[:, :nf]])
        ref[:nf * group] = flash_attn_func_ref(qr[None, None, :nf * group], kk[None], vv[None], **kw)[0, 0]
        kk, vv = torch.cat([sk, kr[None, nf:]]), torch.cat([sv, v[:, nf:]])
        ref[nf * group:] = flash_attn_func_ref(qr[None, None, nf * group:], kk[None], vv[None], **kw)[0, 0]
        attn_close(ob.view[0], ref, "", None)
        assert torch.equal(fvb.view[:full_len + 1].cpu(), torch.cat([fv, v[:, :nf]]))
        assert torch.equal(fkb.view[:full_len].cpu(), fk)
        ek, ev = torch.zeros(W, ns, D, dtype=torch.bfloat16), torch.zeros(W, ns, D, dtype=torch.bfloat16)
        ek[:str_len], ev[:str_len] = sk, sv
        assert OracleBackend().stream_compress(ek, ev, kr[None, nf:], v[:, nf:], str_len, sink, recent) == n_new
        assert torch.equal(svb.view[:n_new].cpu(), ev[:n_new]) and torch.equal(skb.view[:n_new - 1].cpu(), ek[:n_new - 1])


# ============================================================================= 3. prefill
PREFILL_LENS = {None: None, 1: 1, 63: 65, 65: 63, 200: 130, 1100: 200}       # lenA of the retrieval pool -> of the streaming pool
PREFILL_S = [2, 65, 300]


@pytest.mark.parametrize("ksplit", [0, 2, 5], ids=["planned", "k2", "k5"])
@pytest.mark.parametrize("flags", [0, 128, 1024], ids=["w4x64", "w8x32", "plain-order"])
@pytest.mark.parametrize("head_major", [True, False])
def test_prefill(head_major, flags, ksplit):
    """attn_prefill: segment A a view of a larger poisoned pool, q / new rows / out row views of larger buffers with gap
    heads; lenA None is the first chunk (no pools); debug bits 12-15 force the key-range split of the retrieval class"""
    h = _hip()
    with _Flags(flags | (ksplit << 12)):
        for group in (4, 1):
            for lenA, lenS in PREFILL_LENS.items():
                for S in PREFILL_S:
                    _run_bf16_attention(lambda q, out, f, s: h.attn_prefill(q, out, group, f, s, SCALE), group, 2, 1, S,
                                        lenA or 0, lenS or 0, head_major, f"prefill g{group} lenA {lenA} S {S}", seed=S)


def test_prefill_batched():
    _run_bf16_batched(65, 200, 63, "batched prefill")


# ============================================================================= 4. INT4 pools
def _int4_embed(x, cap, head_major=True):
    """x [T, h, 128] fp16 (CPU) -> (packed DeadBuf, scale-zero DeadBuf) holding the oracle's quantisation of x in rows [0, T)"""
    from oracle.int4_oracle import quantize_int4_ref

    p, s, z = quantize_int4_ref(x.float().numpy())
    sz = torch.stack([torch.from_numpy(s), torch.from_numpy(z)], -1)
    return (dead_embed(torch.from_numpy(p), cap=cap, head_major=head_major, device=DEV),
            dead_embed(sz, cap=cap, head_major=head_major, device=DEV, sz=True))


@pytest.mark.parametrize("head_major", [True, False])
@pytest.mark.parametrize("row0", [0, 123])
def test_int4_quantize(row0, head_major):
    """rows outside [row0, row0 + n) of both pools stay unchanged; source rows behind n and its gap heads are poison"""
    from oracle.int4_oracle import quantize_int4_ref

    h = _hip()
    nh, cap = 3, 123 + 70 + 130
    for n in (1, 15, 17, 70):
        g = torch.Generator().manual_seed(n)
        x = (torch.randn(n, nh, D, generator=g) * 2).to(torch.float16)
        xb = dead_embed(x, lead=2, device=DEV)
        qpool = dead_embed(torch.zeros(cap, nh, 64, dtype=torch.uint8), head_major=head_major, tail=0, device=DEV)
        spool = dead_embed(torch.zeros(cap, nh, 2, dtype=torch.float16), head_major=head_major, tail=0, device=DEV)
        qo, so = DeadBuf.guarded(qpool.big, qpool.view[row0:row0 + n]), DeadBuf.guarded(spool.big, spool.view[row0:row0 + n])
        p, s, z = quantize_int4_ref(x.float().numpy())
        zero = None
        for kind in ("zero",) + DEAD_KINDS:
            xb.reset(kind), qo.reset("guard"), so.reset("guard")
            h.int4_quantize(xb.view, qpool.view, spool.view, row0)
            got = _snap(qo.view, so.view)
            qo.assert_dead("guard", what=f"quantize n {n} nibble pool ({kind})")
            so.assert_dead("guard", what=f"quantize n {n} scale-zero pool ({kind})")
            xb.assert_dead(kind, what="quantize source")
            if zero is None:
                zero = got
                assert np.array_equal(qo.view.cpu().numpy(), p)
                assert np.array_equal(so.view.cpu()[..., 0].numpy(), s) and np.array_equal(so.view.cpu()[..., 1].numpy(), z)
            else:
                _same(got, zero, f"quantize n {n} row0 {row0} ({kind})")


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("n,nh", [(1, 1), (50, 3), (300, 4)])
def test_int4_dequantize(n, nh, fused):
    from oracle.int4_oracle import dequantize_int4_ref, quantize_int4_ref

    h = _hip()
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, nh, D, generator=g) * 2).to(torch.float16)
    qb, sb = _int4_embed(x, n + 130)
    big = torch.zeros((n + 260) * nh * D, dtype=torch.float16, device=DEV)
    ob = DeadBuf.guarded(big, big[130 * nh * D:(130 + n) * nh * D])
    want = dequantize_int4_ref(*quantize_int4_ref(x.float().numpy()), fused=fused)
    zero = None
    for kind in ("zero",) + INT4_DEAD_KINDS:
        qb.reset(kind), sb.reset(kind), ob.reset("guard")
        res = h.int4_dequantize(qb.view, sb.view, n, ob.view, fused=fused)
        got = _snap(res)
        ob.assert_dead("guard", what=f"dequantize out ({kind})")
        if zero is None:
            zero = got
            assert np.array_equal(res.cpu().numpy().view(np.uint16), want.view(np.uint16))
        else:
            _same(got, zero, f"dequantize ({kind})")


@pytest.mark.parametrize("length", [5, 12, 13, 40], ids=["below-window", "at-window", "sliding-1", "sliding-28"])
def test_int4_stream_compress(length):
    """in place on all four pools: rows below the new length against the restated move (and the zero run), rows at or behind
    the old length still poison"""
    h = _hip()
    sink, recent, nh = 4, 8, 3
    W = sink + recent
    g = torch.Generator().manual_seed(length)
    x = [(torch.randn(length, nh, D, generator=g) * 2).to(torch.float16) for _ in range(2)]
    (kq, ksz), (vq, vsz) = (_int4_embed(t, max(length, W) + 130) for t in x)
    pools = (kq, ksz, vq, vsz)
    n_new = min(length, W)
    zero = None
    for kind in ("zero",) + INT4_DEAD_KINDS:
        for b in pools:
            b.reset(kind)
        n = h.int4_stream_compress(kq.view, ksz.view, vq.view, vsz.view, length, sink, recent)
        assert n == n_new
        got = _snap(*(b.view[:n] for b in pools))
        for b in pools:
            b.assert_dead(kind, what=f"int4 stream compress, rows behind the old length ({kind})")
        if zero is None:
            zero = got
            for b in pools:
                exp = b.at_live(b.initial).clone()
                if length > W:
                    exp[sink:W] = exp.clone()[length - recent:length]
                assert torch.equal(b.view[:n], exp[:n])
        else:
            _same(got, zero, f"int4 stream compress ({kind})")


@functools.lru_cache(maxsize=None)
def _int4_case(group, T, nf, ns, n_full, n_stream, seed=0):
    """q [T, Hq, 128] fp16, the rows of both pools, and the exact attention over the oracle's dequantised rows in both
    dequantisation forms: token i over rows [0, len - T + i] (test_int4_multi_gpu._ref_multi)"""
    from test_int4_multi_gpu import _dq, _ref_multi

    g = torch.Generator().manual_seed(1000 * T + n_full + group + 7 * seed)
    Hq = (nf + ns) * group
    q = torch.randn(T, Hq, D, generator=g).to(torch.float16)
    rows, refs = [], {f: (torch.empty(T, Hq, D), torch.empty(T, Hq, D)) for f in (0, 1)}
    for n_h, L, off in ((nf, n_full, 0), (ns, n_stream, nf * group)):
        k, v = (torch.randn(L, n_h, D, generator=g).to(torch.float16) for _ in range(2))
        rows.append((k, v))
        sl = slice(off, off + n_h * group)
        for f in (0, 1):
            refs[f][0][:, sl], refs[f][1][:, sl] = _ref_multi(q.float()[:, sl], _dq(k, f), _dq(v, f), group)
    return q, rows, refs


def _run_int4_decode(call, modes, group, T, n_full, n_stream, head_major, what, batch=1):
    """``call(q, out, full, stream, mode)``; q / out [T, Hq, 128] (or [B, T, Hq, 128]) views with gap heads and row slack"""
    from test_int4_multi_gpu import _bar

    h = _hip()
    nf, ns = 2, 1
    cases = [_int4_case(group, T, nf, ns, n_full, n_stream, seed=b) for b in range(batch)]
    one = lambda t: t[0] if batch == 1 else t
    emb = [[[_int4_embed(kv[:n], n + 130, head_major) for kv in c[1][ci]] for c in cases] for ci, n in ((0, n_full), (1, n_stream))]
    pools = []          # per class: kq, ksz, vq, vsz with the batch rows stacked
    for ci in range(2):
        four = []
        for j, sz in ((0, 0), (0, 1), (1, 0), (1, 1)):
            parts = [emb[ci][b][j][sz] for b in range(batch)]
            if batch == 1:
                four.append(parts[0])
                continue
            big = torch.stack([p.big for p in parts])
            view = torch.as_strided(big, (batch,) + tuple(parts[0].view.shape), (big.stride(0),) + tuple(parts[0].view.stride()),
                                    parts[0].view.storage_offset())
            four.append(DeadBuf(big, view, n_live=parts[0].live.shape[0], sz=parts[0].sz))
        pools.append(four)
    qb = dead_embed(one(torch.stack([c[0] for c in cases])), lead=2, device=DEV)
    ob = guard_embed(qb.live.shape, torch.float16, device=DEV)
    bufs = [qb] + [b for four in pools for b in four]
    for mode in modes:
        zero = None
        for kind in ("zero",) + INT4_DEAD_KINDS:
            for b in bufs:
                b.reset(kind)
            ob.reset("guard")
            cls = [h.make_int4_pool(*(b.view for b in four), n, off) for four, n, off in zip(pools, (n_full, n_stream), (0, nf * group))]
            call(qb.view, ob.view, cls[0], cls[1], mode)
            got = _snap(ob.view)
            ob.assert_dead("guard", what=f"{what} mode {mode} out ({kind})")
            if zero is not None:
                _same(got, zero, f"{what} mode {mode} ({kind})")
                continue
            zero = got
            o = ob.view.float().cpu()
            assert torch.isfinite(o).all()
            for b in range(batch):
                ref, bud = cases[b][2][mode & 1]
                ob_ = o[b] if batch > 1 else o
                err, tol = (ob_ - ref).abs(), _bar(ref, bud)
                assert (err <= tol).all(), f"{what} mode {mode}: max err {err.max():.3e}, worst err / tol {float((err / tol.clamp_min(1e-30)).max()):.3f}"


INT4_LENS = [1, 31, 33, 300, 4099]


@pytest.mark.parametrize("group,flags", [(4, 0), (3, 0), (4, 16)], ids=["g4", "g3", "g4-scalar-fma"])
def test_int4_decode(group, flags):
    """attn_decode_int4, modes 0..3 (2 / 3: the folded kernel); debug bit 4 forces the scalar-FMA kernel"""
    h = _hip()
    with _Flags(flags):
        for L in INT4_LENS:
            _run_int4_decode(lambda q, out, f, s, mode: h.attn_decode_int4(q[0], out[0], group, f, s, SCALE, fused=mode),
                             (0, 1, 2, 3) if not flags else (0, 1), group, 1, L, min(L, 20), True, f"int4 decode g{group} len {L}")


@pytest.mark.parametrize("group,T,head_major", [(g, T, True) for g in (4, 3, 16) for T in (2, 5, 16, 64)] + [(4, 5, False)])
def test_int4_decode_multi(group, T, head_major):
    h = _hip()
    for L in (T, T + 31, 300, 4099):
        _run_int4_decode(lambda q, out, f, s, mode: h.attn_decode_int4_multi(q, out, group, f, s, SCALE, fused=mode),
                         (0, 1), group, T, L, T + min(L - T, 20), head_major, f"int4 multi g{group} T {T} len {L}")


def test_int4_decode_multi_batched():
    """B = 2, both (fused & 1) values; `out` is padded: its batch rows are more than T token strides apart"""
    h = _hip()
    _run_int4_decode(lambda q, out, f, s, mode: h.attn_decode_int4_multi_batched(q, out, 4, f, s, SCALE, fused=mode),
                     (0, 1), 4, 5, 4099, 385, True, "int4 multi batched", batch=2)


# ============================================================================= 5. tuple path
@pytest.mark.parametrize("n,full_len", [(5, 37), (64, 300), (63, 0)])
def test_tuple_prep_then_attention(n, full_len):
    """tuple_decode_prep then attn_decode_tuple: arena rows behind full_len + 1 and streaming source rows behind its length are
    poison; arena rows the step does not write stay unchanged"""
    from oracle.duo_oracle import flash_attn_func_ref, tuple_decode_prep_ref

    h = _hip()
    nf, ns, group, sink, recent = 2, 2, 4, 16, 48
    nkv, Hq = nf + ns, (nf + ns) * group
    g = torch.Generator().manual_seed(n + full_len)
    q, k, v = _rand((1, Hq, D), g), _rand((1, nkv, D), g), _rand((1, nkv, D), g)
    ang = torch.rand(D // 2, generator=g) * 6.28
    cos, sin = (torch.cat([f(ang), f(ang)]).to(torch.bfloat16) for f in (torch.cos, torch.sin))
    arena_live, src_live = _rand((2, full_len, nf, D), g), _rand((2, n, ns, D), g)
    # [2, heads, rows, D] arena / streaming source = the head-major embedding with the K / V pair as the batch dimension
    ab = dead_embed(arena_live, cap=full_len + 1 + 130, tail=0, gap=0, head_major=True, device=DEV)
    sb = dead_embed(src_live, cap=n, tail=130, gap=0, head_major=True, device=DEV)
    arena = ab.view.transpose(1, 2)                                    # [2, nf, cap, D]
    src = sb.view.transpose(1, 2)                                      # [2, ns, n, D], 130 poison rows behind every head
    qb, kb, vb = (dead_embed(t, lead=2, device=DEV) for t in (q, k, v))
    ob = guard_embed((1, Hq, D), torch.bfloat16, device=DEV)
    zero = None
    for kind in ("zero",) + DEAD_KINDS:
        for b in (ab, sb, qb, kb, vb):
            b.reset(kind)
        ob.reset("guard")
        new = h.tuple_decode_prep(qb.view[0], kb.view[0], vb.view[0], cos.to(DEV), sin.to(DEV), nf, arena, full_len, src, sink, recent)
        h.attn_decode_tuple(qb.view[0], ob.view[0], group, nf, arena, full_len, src, kb.view[0], vb.view[0], SCALE)
        got = _snap(ob.view, new, ab.view[:, :full_len + 1], qb.view, kb.view)
        ob.assert_dead("guard", what=f"tuple out ({kind})")
        ab.assert_dead(kind, live=ab.view[:, :full_len + 1], what=f"arena rows the step does not write ({kind})")
        sb.assert_dead(kind, what=f"streaming source ({kind})")
        for b in (qb, kb, vb):
            b.assert_dead(kind, what=f"tuple q / k / v gaps ({kind})")
        if zero is not None:
            _same(got, zero, f"tuple step ({kind})")
            continue
        zero = got
        rq, rk, rv = q[0].clone(), k[0].clone(), v[0].clone()
        r_arena = torch.zeros(2, nf, full_len + 1, D, dtype=torch.bfloat16)
        r_arena[:, :, :full_len] = arena_live.transpose(1, 2)
        want = tuple_decode_prep_ref(rq, rk, rv, cos, sin, nf, r_arena, full_len, src_live.transpose(1, 2), sink, recent)
        assert torch.equal(new.cpu(), want) and torch.equal(arena[:, :, :full_len + 1].cpu(), r_arena)
        assert torch.equal(qb.view[0].cpu(), rq) and torch.equal(kb.view[0].cpu(), rk)
        ref = torch.empty(Hq, D)
        kw = dict(round_p=False, out_dtype=torch.float32)
        kk, vv = r_arena[0].transpose(0, 1), r_arena[1].transpose(0, 1)
        ref[:nf * group] = flash_attn_func_ref(rq[None, None, :nf * group], kk[None], vv[None], **kw)[0, 0]
        kk = torch.cat([src_live[0], rk[None, nf:]])
        vv = torch.cat([src_live[1], rv[None, nf:]])
        ref[nf * group:] = flash_attn_func_ref(rq[None, None, nf * group:], kk[None], vv[None], **kw)[0, 0]
        attn_close(ob.view[0], ref, "", None)


# ============================================================================= 6. Λ-mask training attention
def _lambda_raw(h, q, k, v, dout, ps, pr, mode, outs):
    """duo_lambda_attn_fwd_bf16 (and, with ``dout``, duo_lambda_attn_bwd_bf16) through the C ABI, as duo_attn._hip calls them,
    writing into the caller's (guarded, contiguous) out / lse / dq / dk / dv"""
    lib = h.load_library()
    B, S, Hq, _ = q.shape
    Hkv = k.shape[2]
    strides = lambda t: (t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))
    out, lse = outs["out"].view, outs["lse"].view
    assert lib.duo_lambda_attn_fwd_bf16(*strides(q), *strides(k), *strides(v), out.data_ptr(), lse.data_ptr(), B, S, Hq, Hkv, D,
                                        ps, pr, mode, SCALE, h._stream_ptr()) == 0
    if dout is None:
        return
    nbytes = int(lib.duo_lambda_attn_bwd_workspace_bytes(B, S, Hq, Hkv, ps, pr, mode))
    assert nbytes >= 0
    ws = torch.empty((nbytes + 15) // 16 * 4, dtype=torch.float32, device=DEV)
    assert all(st % 8 == 0 for st in dout.stride()[:3]) and dout.data_ptr() % 16 == 0
    assert lib.duo_lambda_attn_bwd_bf16(*strides(q), *strides(k), *strides(v), out.data_ptr(), *strides(dout), lse.data_ptr(),
                                        outs["dq"].view.data_ptr(), outs["dk"].view.data_ptr(), outs["dv"].view.data_ptr(),
                                        ws.data_ptr(), ws.numel() * 4, B, S, Hq, Hkv, D, ps, pr, mode, SCALE, h._stream_ptr()) == 0
    torch.cuda.synchronize()        # (the workspace is freed on return)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("sink,recent", [(64, 128), (100, 37)])
@pytest.mark.parametrize("heads", [(8, 2), (4, 1)])
def test_lambda_attention(heads, sink, recent, mode):
    """lambda_attn_fwd / lambda_attn_bwd, B = 2: q, k, v and dout are views with poison rows behind S inside each batch row and
    poisoned gap heads; out, lse, dq, dk, dv bit-equal across poison kinds (dK / dV sum over query rows: a poisoned q or dout
    row behind S would surface there).  The kernels are called through the C ABI (the Python binding allocates its outputs
    itself): out, lse, dq, dk and dv lie inside 130 guard rows either side.  The zero run: out at attn_close, lse at
    test_lambda_attn_gpu's bar (2 x the fp32 reference's own maximum error against fp64), the gradients at 1.25 x the FA2
    reference arithmetic's rms error."""
    from test_lambda_attn_gpu import _params
    from training_ref import attention_budget, dense_attention, dense_grads, fa2_reference, lambda_mask, rms

    h = _hip()
    Hq, Hkv = heads
    ps, pr = _params(sink, recent, mode)
    for S in (1, 63, 65, 129, 200):
        g = torch.Generator().manual_seed(S)
        q, dout = _rand((2, S, Hq, D), g), _rand((2, S, Hq, D), g)
        k, v = _rand((2, S, Hkv, D), g), _rand((2, S, Hkv, D), g)
        bufs = [dead_embed(t, lead=2, device=DEV) for t in (q, k, v, dout)]
        qb, kb, vb, db = bufs
        outs = {n: guard_flat(shape, dt, 130 * shape[-2] * shape[-1] if dt == torch.bfloat16 else 130 * S)
                for n, shape, dt in (("out", (2, S, Hq, D), torch.bfloat16), ("lse", (2, Hq, S), torch.float32),
                                     ("dq", (2, S, Hq, D), torch.bfloat16), ("dk", (2, S, Hkv, D), torch.bfloat16),
                                     ("dv", (2, S, Hkv, D), torch.bfloat16))}
        zero = None
        for kind in ("zero",) + DEAD_KINDS:
            for b in bufs:
                b.reset(kind)
            for b in outs.values():
                b.reset("guard")
            _lambda_raw(h, qb.view, kb.view, vb.view, db.view if S > 1 else None, ps, pr, mode, outs)
            out, lse = outs["out"].view, outs["lse"].view
            res = [outs[n].view for n in (("out", "lse", "dq", "dk", "dv") if S > 1 else ("out", "lse"))]
            got = _snap(*res)
            for n, b in outs.items():
                b.assert_dead("guard", what=f"lambda {n} S {S} ({kind})")
            for b in bufs:
                b.assert_dead(kind, what=f"lambda inputs S {S} ({kind})")
            if zero is not None:
                _same(got, zero, f"lambda S {S} H{Hq}/{Hkv} sink{ps} recent{pr} mode{mode} ({kind})")
                continue
            zero = got
            mask = lambda_mask(S, ps, pr, mode, DEV)
            qd, kd, vd, dd = (t.to(DEV) for t in (q, k, v, dout))
            ref, _ = dense_attention(qd, kd, vd, mask, dtype=torch.float32)
            ref_r, _ = dense_attention(qd, kd, vd, mask, dtype=torch.float32, round_p=True)
            attn_close(out.float(), ref, "", budget=with_rounded(attention_budget(qd, kd, vd, mask), ref_r.to(torch.bfloat16).float()))
            _, lse64 = dense_attention(qd, kd, vd, mask, dtype=torch.float64)
            _, lse32 = dense_attention(qd, kd, vd, mask, dtype=torch.float32)
            e_hip, e_ref = float((lse.double() - lse64).abs().max()), float((lse32.double() - lse64).abs().max())
            print(f"lambda lse S {S}: max err {e_hip:.3e}, fp32 reference {e_ref:.3e}")
            assert e_hip <= 2 * e_ref, f"S {S}: lse max err {e_hip:.3e} > 2 x fp32 reference's {e_ref:.3e}"
            if S > 1:
                truth, fa2 = dense_grads(qd, kd, vd, dd, mask, dtype=torch.float64), fa2_reference(qd, kd, vd, dd, mask)
                for name, x, t, r in zip(("dq", "dk", "dv"), res[2:], truth, fa2):
                    e_hip, e_ref = rms(x.double() - t), rms(r.double() - t)
                    print(f"lambda bwd {name} S {S}: rms err {e_hip:.3e}, reference arithmetic {e_ref:.3e}")
                    assert e_hip <= 1.25 * e_ref, f"{name} S {S}: rms err {e_hip:.3e} > 1.25 x reference arithmetic's {e_ref:.3e}"


# ============================================================================= 7. row kernels
ROW_SIZES = [(1, 4096), (33, 4096), (7, 1032)]


@pytest.mark.parametrize("S", [1, 33, 7])
def test_rope_inplace_rows(S):
    from oracle.duo_oracle import rope_ref
    from test_hip_kernels_gpu import _ulp_close

    h = _hip()
    g = torch.Generator().manual_seed(S)
    q, k = _rand((S, 8, D), g), _rand((S, 2, D), g)
    qb, kb = dead_embed(q, lead=130, device=DEV), dead_embed(k, lead=130, device=DEV)
    zero = None
    for kind in ("zero",) + DEAD_KINDS:
        qb.reset(kind), kb.reset(kind)
        h.rope_inplace(qb.view, kb.view, 1000, 1.0, 5e5)
        got = _snap(qb.view, kb.view)
        qb.assert_dead(kind, what=f"rope q ({kind})"), kb.assert_dead(kind, what=f"rope k ({kind})")
        if zero is None:
            zero = got
            _ulp_close(qb.view, rope_ref(q, 1000, 1.0, 5e5), "rope q")
            _ulp_close(kb.view, rope_ref(k, 1000, 1.0, 5e5), "rope k")
        else:
            _same(got, zero, f"rope ({kind})")


@pytest.mark.parametrize("S", [1, 33, 7])
def test_rope_hf_inplace_rows(S):
    """cos / sin rows are strided views too (poison between them and behind S)"""
    h = _hip()
    g = torch.Generator().manual_seed(S)
    q, k = _rand((S, 8, D), g), _rand((S, 2, D), g)
    ang = torch.rand(S, D // 2, generator=g) * 6.28
    cos, sin = (torch.cat([f(ang), f(ang)], -1).to(torch.bfloat16) for f in (torch.cos, torch.sin))
    qb, kb = dead_embed(q, lead=130, device=DEV), dead_embed(k, lead=130, device=DEV)
    cb, sb = _row2d(cos), _row2d(sin)
    rot = lambda x: torch.cat([-x[..., D // 2:], x[..., :D // 2]], -1)
    want = [x * cos[:, None] + rot(x) * sin[:, None] for x in (q, k)]       # torch's bf16 arithmetic, as HF runs it
    zero = None
    for kind in ("zero",) + DEAD_KINDS:
        for b in (qb, kb, cb, sb):
            b.reset(kind)
        h.rope_hf_inplace(qb.view, kb.view, cb.view[:, 0], sb.view[:, 0])
        got = _snap(qb.view, kb.view)
        for b in (qb, kb, cb, sb):
            b.assert_dead(kind, what=f"rope_hf ({kind})")
        if zero is None:
            zero = got
            assert torch.equal(qb.view.cpu(), want[0]) and torch.equal(kb.view.cpu(), want[1])
        else:
            _same(got, zero, f"rope_hf ({kind})")


@pytest.mark.parametrize("hf", [False, True], ids=["rmsnorm", "rmsnorm_hf"])
@pytest.mark.parametrize("rows,hidden", ROW_SIZES)
def test_rmsnorm_rows(rows, hidden, hf):
    """duo_rmsnorm[_hf]_bf16 take contiguous rows (no stride): poison rows behind n_rows, `y` inside guard rows"""
    from oracle.duo_oracle import rmsnorm_hf_ref, rmsnorm_ref
    from test_hip_kernels_gpu import _ulp_close

    h = _hip()
    lib = h.load_library()
    g = torch.Generator().manual_seed(rows)
    x, w = _rand((rows, hidden), g) * 3, _rand((hidden,), g)
    xb = dead_embed(x[:, None, :], lead=0, tail=3, gap=0, device=DEV)
    yb = guard_embed((rows, 1, hidden), torch.bfloat16, gap=0, device=DEV)
    wd = w.to(DEV)
    fn = lib.duo_rmsnorm_hf_bf16 if hf else lib.duo_rmsnorm_bf16
    zero = None
    for kind in ("zero",) + DEAD_KINDS:
        xb.reset(kind), yb.reset("guard")
        assert fn(xb.view.data_ptr(), wd.data_ptr(), yb.view.data_ptr(), rows, hidden, 1e-5, h._stream_ptr()) == 0
        got = _snap(yb.view)
        yb.assert_dead("guard", what=f"rmsnorm y ({kind})"), xb.assert_dead(kind, what="rmsnorm x")
        if zero is None:
            zero = got
            _ulp_close(yb.view[:, 0], (rmsnorm_hf_ref if hf else rmsnorm_ref)(x, w, 1e-5), "rmsnorm", max_frac=0.02)
        else:
            _same(got, zero, f"rmsnorm ({kind})")


@pytest.mark.parametrize("rows,n", ROW_SIZES)
def test_silu_mul_rows(rows, n):
    h = _hip()
    lib = h.load_library()
    g = torch.Generator().manual_seed(rows)
    gate, up = _rand((rows, n), g), _rand((rows, n), g)
    gb, ub = _row2d(gate), _row2d(up)
    yb = guard_embed((rows, 1, n), torch.bfloat16, gap=1, device=DEV)
    want = (torch.nn.functional.silu(gate.float()).to(torch.bfloat16).float() * up.float()).to(torch.bfloat16).float()
    zero = None
    for kind in ("zero",) + DEAD_KINDS:
        gb.reset(kind), ub.reset(kind), yb.reset("guard")
        gv, uv, yv = gb.view[:, 0], ub.view[:, 0], yb.view[:, 0]
        assert lib.duo_silu_mul_bf16(gv.data_ptr(), gv.stride(0), uv.data_ptr(), uv.stride(0), yv.data_ptr(), yv.stride(0),
                                     rows, n, h._stream_ptr()) == 0
        got = _snap(yv)
        yb.assert_dead("guard", what=f"silu_mul y ({kind})")
        if zero is None:
            zero = got
            # the bar of test_silu_mul_is_the_module_sequence: one bf16 ulp of the fp32 restatement of HF's module sequence
            err = (yv.float().cpu() - want).abs()
            assert (err <= 2.0 ** -7 * want.abs() + 1e-30).all(), float(err.max())
        else:
            _same(got, zero, f"silu_mul ({kind})")


def _token_linear_raw(h, x, blocks, y, norm=None, x2=None, residual=None, norm_hf=False):
    """duo_token_linear_bf16 as duo_attn._hip.token_linear calls it, writing into the caller's y [rows, sum n] (any row stride)"""
    from ctypes import byref

    a = h.TokenLinearArgs()
    a.x, a.x_row_stride, a.n_rows, a.n_in = x.data_ptr(), x.stride(0), x.shape[0], x.shape[1]
    if x2 is not None:
        a.x2 = x2.data_ptr()
    for i, (w, b) in enumerate(blocks):
        a.seg[i].w, a.seg[i].row_stride, a.seg[i].n = w.data_ptr(), w.stride(0), w.shape[0]
        if b is not None:
            a.seg[i].bias = b.data_ptr()
    if norm is not None:
        a.norm_weight, a.norm_eps, a.flags = norm[0].data_ptr(), float(norm[1]), h.LINEAR_NORM_HF if norm_hf else 0
    if residual is not None:
        a.residual, a.residual_row_stride = residual.data_ptr(), residual.stride(0)
    assert y.shape == (x.shape[0], sum(w.shape[0] for w, _ in blocks)) and y.stride(1) == 1
    a.y, a.y_row_stride = y.data_ptr(), y.stride(0)
    assert h.load_library().duo_token_linear_bf16(byref(a), h._stream_ptr()) == 0


@pytest.mark.parametrize("rows,n_in", [(1, 4096), (4, 4096), (3, 1032)])
def test_token_linear_rows(rows, n_in):
    """x (and x2) rows and the residual rows are strided views with poison between them and behind n_rows; `y` is a strided view
    inside guard rows (duo_token_linear_bf16 through the C ABI: the Python binding allocates y itself)"""
    from oracle.duo_oracle import token_linear_ref
    from test_token_linear_gpu import _close

    h = _hip()
    g = torch.Generator().manual_seed(rows + n_in)
    rn = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(torch.bfloat16)
    x, x2, nw = rn(rows, n_in, sc=3.0), rn(rows, n_in), (torch.rand(n_in, generator=g) + 0.5).to(torch.bfloat16)
    blocks = [(rn(384, n_in, sc=n_in ** -0.5), None), (rn(128, n_in, sc=n_in ** -0.5), rn(128))]
    res = rn(rows, 512)
    xb, x2b, rb = _row2d(x), _row2d(x2), _row2d(res)
    yb = guard_embed((rows, 1, 512), torch.bfloat16, gap=1, device=DEV)        # y rows three rows' worth of elements apart
    dblocks = [(w.to(DEV), None if b is None else b.to(DEV)) for w, b in blocks]
    forms = {"norm": dict(norm=(nw, 1e-5)), "norm_hf": dict(norm=(nw, 1e-5), norm_hf=True), "silu": dict(x2=x2), "plain": {}}
    for name, kw in forms.items():
        dkw = dict(kw)
        if "norm" in kw:
            dkw["norm"] = (nw.to(DEV), 1e-5)
        zero = None
        for kind in ("zero",) + DEAD_KINDS:
            xb.reset(kind), x2b.reset(kind), rb.reset(kind)
            if "x2" in kw:
                dkw["x2"] = x2b.view[:, 0]
            yb.reset("guard")
            y = yb.view[:, 0]
            _token_linear_raw(h, xb.view[:, 0], dblocks, y, residual=rb.view[:, 0], **dkw)
            got = _snap(y)
            yb.assert_dead("guard", what=f"token_linear {name} y ({kind})")
            for b in (xb, x2b, rb):
                b.assert_dead(kind, what=f"token_linear {name} inputs ({kind})")
            if zero is None:
                zero = got
                want, pre = token_linear_ref(x, blocks, residual=res, exact=True, **kw)
                _close(y, want, pre, f"token_linear {name}", residual=res)
            else:
                _same(got, zero, f"token_linear {name} ({kind})")


# ============================================================================= 8. caches, end to end
def _slack_pool(batch, rows, heads, X, dtype, pad4=False):
    """a cache pool of ``rows`` logical rows, [B, rows, heads, X] head-major like the caches' own, with >= 130 spare rows
    behind every head inside the allocation -> (the whole buffer, the pool view)"""
    total = ((rows + 3) // 4 * 4 if pad4 else rows) + 132
    big = torch.zeros(batch, heads, total, X, dtype=dtype, device=DEV)
    return big, big.permute(0, 2, 1, 3)[:, :rows]


def _poison_all(bigs, kind):
    for b, sz in bigs:
        b.copy_(dead_values(b.shape, b.dtype, kind, DEV, sz))


CACHE_COUNTS, CACHE_HQ, CACHE_HKV, CACHE_SINK, CACHE_RECENT, CACHE_MAX = [1, 3, 0, 4], 16, 4, 4, 12, 64


def _static_cache_run(kind, use_graph):
    """the protocol of test_hip_kernels_gpu._decode_loop_setup on a cache whose pools were overwritten with ``kind`` right
    after construction and again after clear(): chunked prefill 13, 9 steps, clear(), a longer prompt (29 + 12), 4 steps,
    evict_last(3), 2 steps -> every output, the counters, the device state, the live rows (all as bits)"""
    from duo_attn.graph import DecodeStepGraph
    from duo_attn.patch._duo import duo_static_attention_core
    from duo_attn.patch.static_kv_cache import DuoAttentionStaticKVCache
    from helpers import ShapeModel, heads_from_counts

    L, Hq, Hkv = len(CACHE_COUNTS), CACHE_HQ, CACHE_HKV
    cache = DuoAttentionStaticKVCache(ShapeModel(L, Hq, Hkv, D, device=DEV), heads_from_counts(CACHE_COUNTS, Hkv), 1, CACHE_MAX,
                                      CACHE_SINK, CACHE_RECENT)
    bigs = []
    for lst, rows in ((cache.full_key_states_list, CACHE_MAX), (cache.full_value_states_list, CACHE_MAX),
                      (cache.streaming_key_states_list, CACHE_SINK + CACHE_RECENT),
                      (cache.streaming_value_states_list, CACHE_SINK + CACHE_RECENT)):
        for li in range(L):
            assert lst[li].shape[1] == rows
            big, lst[li] = _slack_pool(1, rows, lst[li].shape[2], D, torch.bfloat16)
            bigs.append((big, False))
    _poison_all(bigs, kind)
    g = torch.Generator().manual_seed(21)
    mk = lambda S, h: _rand((1, S, h, D), g).to(DEV)
    record = []

    def prefill(S):
        pos = cache.kv_seq_len
        for li in range(L):
            record.append(duo_static_attention_core(mk(S, Hq), mk(S, Hkv), mk(S, Hkv), cache, li, pos, 1.0, 1e4))

    prefill(13)
    qs, ks, vs = [mk(1, Hq) for _ in range(L)], [mk(1, Hkv) for _ in range(L)], [mk(1, Hkv) for _ in range(L)]
    outs = [torch.zeros(1, 1, Hq, D, dtype=torch.bfloat16, device=DEV) for _ in range(L)]

    def step():
        pos = cache.kv_seq_len
        for li in range(L):
            outs[li].copy_(duo_static_attention_core(qs[li], ks[li], vs[li], cache, li, pos, 1.0, 1e4))
        return outs

    graph = DecodeStepGraph(cache, step, evict_after=0) if use_graph else None

    def steps(n):
        for _ in range(n):
            graph.replay() if use_graph else step()
            torch.cuda.synchronize()
            record.extend(o.clone() for o in outs)

    steps(9)
    cache.clear()
    _poison_all(bigs, kind)
    prefill(29)
    prefill(12)
    steps(4)
    cache.evict_last(3)
    steps(2)
    res = _snap(*record)
    res.append(torch.tensor([cache.kv_seq_len_list, cache.streaming_kv_seq_len_list]))
    if use_graph:
        res.append(cache.device_state.cpu().clone())
    for li in range(L):
        n, m = cache.kv_seq_len_list[li], cache.streaming_kv_seq_len_list[li]
        res += _snap(cache.full_key_states_list[li][:, :n], cache.full_value_states_list[li][:, :n],
                     cache.streaming_key_states_list[li][:, :m], cache.streaming_value_states_list[li][:, :m])
    return res


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_static_cache_with_poisoned_pools(use_graph):
    zero = _static_cache_run("zero", use_graph)
    assert all(torch.isfinite(o.view(torch.bfloat16).float()).all() for o in zero[:4 * 3 + 4 * 15])
    for kind in DEAD_KINDS:
        _same(_static_cache_run(kind, use_graph), zero, f"static cache, {'graph' if use_graph else 'eager'} ({kind})")


def _int4_cache_run(kind, multi):
    """DuoAttentionStaticINT4KVCache with every packed pool overwritten with ``kind`` after construction and after clear():
    put / attention / compress per layer over chunks 13, nine single tokens, clear(), 29, 12, steps of 3, 1 and 4 tokens,
    evict_last(3), 2 and 1 tokens"""
    from duo_attn.int4_kv import DuoAttentionStaticINT4KVCache
    from helpers import ShapeModel, heads_from_counts

    L, Hq, Hkv = len(CACHE_COUNTS), CACHE_HQ, CACHE_HKV
    model = ShapeModel(L, Hq, Hkv, D, device=DEV, dtype=torch.float16)
    cache = DuoAttentionStaticINT4KVCache(model, heads_from_counts(CACHE_COUNTS, Hkv), 1, CACHE_MAX, CACHE_SINK, CACHE_RECENT, 32,
                                          multi_token_decode=multi)
    bigs = []
    groups = (cache.full_key_caches, cache.full_value_caches, cache.streaming_key_caches, cache.streaming_value_caches)
    for lst in groups:
        for c in lst:
            rows, heads = c.quantized_data.shape[1], c.quantized_data.shape[2]
            qbig, c.quantized_data = _slack_pool(1, rows, heads, 64, torch.uint8, pad4=True)
            sbig, c.scale_zero = _slack_pool(1, rows, heads, 2, torch.float16, pad4=True)
            c.scale, c.zero_point = c.scale_zero[..., 0:1], c.scale_zero[..., 1:2]
            bigs += [(qbig, False), (sbig, True)]
    _poison_all(bigs, kind)
    g = torch.Generator().manual_seed(22)
    record = []

    def run(S):
        for li in range(L):
            q, k, v = (torch.randn(1, S, h, D, generator=g).to(torch.float16).to(DEV) for h in (Hq, Hkv, Hkv))
            was_empty = cache.kv_seq_len_list[li] == 0
            cache.put(li, k, v, dequantize=False)
            if S == 1:
                record.append(cache.decode_attention(li, q))
            elif multi and not was_empty:
                record.append(cache.multi_token_attention(li, q))
            else:
                record.append(cache.prefill_attention(li, q, k, v))
            cache.compress(li)

    for S in (13,) + (1,) * 9:
        run(S)
    cache.clear()
    _poison_all(bigs, kind)
    for S in (29, 12, 3, 1, 4):
        run(S)
    cache.evict_last(3)
    for S in (2, 1):
        run(S)
    res = _snap(*record)
    res.append(torch.tensor([cache.kv_seq_len_list, cache.streaming_kv_seq_len_list]))
    for li in range(L):
        for lst, n in zip(groups, (cache.kv_seq_len_list[li],) * 2 + (cache.streaming_kv_seq_len_list[li],) * 2):
            res += _snap(lst[li].quantized_data[:, :n], lst[li].scale_zero[:, :n])
    return res


@pytest.mark.parametrize("multi", [False, True], ids=["plain", "multi-token-decode"])
def test_int4_cache_with_poisoned_pools(multi):
    zero = _int4_cache_run("zero", multi)
    assert all(torch.isfinite(o.view(torch.float16).float()).all() for o in zero[:4 * 17])
    for kind in INT4_DEAD_KINDS:
        _same(_int4_cache_run(kind, multi), zero, f"int4 cache multi={multi} ({kind})")


class _CountingBackend:
    """the HIP backend, counting the fused tuple step's launches (so the case below knows the fused form really ran)"""

    def __init__(self, inner):
        self.inner, self.n_prep, self.n_attn = inner, 0, 0

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def tuple_decode_prep(self, *a, **kw):
        self.n_prep += 1
        return self.inner.tuple_decode_prep(*a, **kw)

    def tuple_decode_attention(self, *a, **kw):
        self.n_attn += 1
        return self.inner.tuple_decode_attention(*a, **kw)


def _tuple_model_run(base, kind):
    """a patched tiny Llama on the tuple path.  After EVERY forward — the prefill, each decode step, the step that re-allocates
    the arena (an older tuple re-used for a branch is copied into a fresh one), the longer prompt after release_tuple_arena —
    rows [len, capacity) of every layer's arena (>= 1024 of them) are overwritten with ``kind``.  (The streaming tuples are
    fresh tensors of exactly their length: there is nothing behind them.)  -> logits of every call, the returned past of the
    last one, the arenas' live rows, as bits"""
    import copy

    from duo_attn import backend
    from duo_attn.patch import enable_duo_attention_eval
    from duo_attn.patch._duo import release_tuple_arena

    model = copy.deepcopy(base)
    heads = np.array([[0.0, 1.0], [1.0, 1.0], [0.0, 0.0]])
    enable_duo_attention_eval(model, heads.copy(), 16, 48)         # window 64: grows, fills and slides in the steps below
    ids = torch.randint(0, 211, (1, 120), generator=torch.Generator().manual_seed(12)).to(DEV)
    rec = _CountingBackend(backend.HipBackend())
    backend._set_backend_for_testing(rec)
    logits, seen = [], set()

    def poison():
        for layer in model.model.layers:
            a = getattr(layer.self_attn, "_duo_full_kv_arena", None)
            if a is not None and a["buf"].shape[1] > 0:
                seen.add(a["buf"].data_ptr())
                assert a["buf"].shape[2] - a["len"] >= 130
                dead = a["buf"][:, :, a["len"]:]
                dead.copy_(dead_values(dead.shape, dead.dtype, kind, DEV))

    def call(lo, hi, past):
        o = model(input_ids=ids[:, lo:hi], past_key_values=past, use_cache=True)
        poison()
        logits.append(o.logits)
        return o.past_key_values

    try:
        with torch.no_grad():
            p0 = call(0, 58, None)
            past = p0
            for t in range(58, 66):                 # the streaming window (64) fills and starts to slide
                past = call(t, t + 1, past)
            n_arenas = len(seen)
            past = call(70, 71, p0)                 # a branch from the older tuple: copied into fresh arenas
            assert len(seen) > n_arenas
            for t in range(71, 74):
                past = call(t, t + 1, past)
            release_tuple_arena(model)
            past = call(0, 90, None)                # a longer prompt
            for t in range(90, 96):
                past = call(t, t + 1, past)
    finally:
        backend._set_backend_for_testing(None)
    assert rec.n_prep == rec.n_attn == 3 * (8 + 4 + 6), (rec.n_prep, rec.n_attn)      # every decode step took the fused form
    res = _snap(*logits)
    for (full, stream), layer in zip(past, model.model.layers):
        res += _snap(full, stream)
        a = getattr(layer.self_attn, "_duo_full_kv_arena", None)
        assert full.shape[2] == 96
        if full.numel():
            assert a["len"] == 96 and full.data_ptr() == a["buf"].data_ptr()
            res += _snap(a["buf"][:, :, :a["len"]])
    return res


def test_tuple_arena_with_poisoned_rows():
    """the fused tuple decode step as the patched forward wires it (strides, full_capacity, the arena's length bookkeeping):
    logits of every call, the returned past views and the arenas' live rows are bit-equal to a twin whose dead arena rows are
    zero; the twin's decode path against HF eager is test_tuple_decode_gpu's subject"""
    from test_golden_and_model_gpu import tiny

    base = tiny("llama", seed=11)
    zero = _tuple_model_run(base, "zero")
    assert all(torch.isfinite(x.view(torch.bfloat16).float()).all() for x in zero[:20])
    for kind in DEAD_KINDS:
        _same(_tuple_model_run(base, kind), zero, f"tuple path, arena rows behind len ({kind})")
