"""GPU: decode steps of 2..64 tokens over the bf16 pools on the split-KV matrix-core stream (duo_decode_multi_kernel).

Parity is held to the project's prefill bars (helpers.attn_close with the P-rounding budget and the reference arithmetic's own
noise, the 1.12 ratio included) against oracle.duo_oracle.flash_attn_func_ref; the mask, the dead rows, the guard bytes and
the bit-equalities need no tolerance at all.  Shapes are the smallest at which the kernel's paths differ: 32-key tiles, four
waves per workgroup, 64-key split units, 16 / group tokens per column block.
"""
import functools
import math

import pytest
import torch

from helpers import (DEAD_KINDS, ShapeModel, _bits, attn_close, dead_embed, guard_embed, heads_from_counts, with_rounded)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 128
SCALE = D ** -0.5


def _hip():
    from duo_attn import _hip

    _hip.load_library()
    return _hip


def _rand(shape, gen):
    return torch.randn(shape, generator=gen).to(torch.bfloat16)


def _snap(*tensors):
    torch.cuda.synchronize()
    return [_bits(t).cpu().clone() for t in tensors]


@functools.lru_cache(maxsize=None)
def _case(group, T, nf, ns, lenF, lenS, seed=0):
    """live data (CPU) of one step + the oracle's answers: q [T, Hq, D], new rows [T, nkv, D], pools [len, n_h, D] or None,
    the exact-P fp32 reference and its budget carrying the reference arithmetic's own (rounded-P, bf16) result"""
    from oracle.duo_oracle import flash_attn_func_ref

    g = torch.Generator().manual_seed(1000 * seed + 17 * T + group)
    nkv, Hq = nf + ns, (nf + ns) * group
    q, kn, vn = _rand((T, Hq, D), g), _rand((T, nkv, D), g), _rand((T, nkv, D), g)
    pools = []
    ref, bud, rnd = (torch.empty(T, Hq, D) for _ in range(3))
    for lo, n_h, L in ((0, nf, lenF), (nf, ns, lenS)):
        pk, pv = (_rand((L, n_h, D), g), _rand((L, n_h, D), g)) if n_h and L else (None, None)
        pools.append((pk, pv))
        if n_h == 0:
            continue
        kk = torch.cat([pk, kn[:, lo:lo + n_h]]) if L else kn[:, lo:lo + n_h]
        vv = torch.cat([pv, vn[:, lo:lo + n_h]]) if L else vn[:, lo:lo + n_h]
        sl = slice(lo * group, (lo + n_h) * group)
        r, b = flash_attn_func_ref(q[None, :, sl], kk[None], vv[None], round_p=False, out_dtype=torch.float32, return_budget=True)
        ref[:, sl], bud[:, sl] = r[0], b[0]
        rnd[:, sl] = flash_attn_func_ref(q[None, :, sl], kk[None], vv[None], round_p=True, out_dtype=torch.bfloat16)[0]
    return q, kn, vn, pools, ref, with_rounded(bud, rnd)


def _pool_to_dev(t, head_major):
    """[len, n_h, D] on the device, rows head-major (the cache's layout) or token-major (the reference's)"""
    if t is None:
        return None
    return t.transpose(0, 1).contiguous().to(DEV).transpose(0, 1) if head_major else t.to(DEV)


def _classes(h, group, nf, ns, pools, kn, vn):
    """pools: per class (k, v) device views [(B,) len, n_h, D] or (None, None); kn / vn [(B,) T, nkv, D] device views"""
    cls = []
    for (lo, n_h), (pk, pv) in zip(((0, nf), (nf, ns)), pools):
        segA = h.make_seg(pk, pv) if pk is not None else h.make_seg(None, None)
        cls.append(h.make_class(n_h, lo * group, segA, h.make_seg(kn[..., lo:lo + n_h, :], vn[..., lo:lo + n_h, :])) if n_h else None)
    return cls


def _run(group, T, nf, ns, lenF, lenS, head_major=True, seed=0):
    h = _hip()
    q, kn, vn, pools, ref, bud = _case(group, T, nf, ns, lenF, lenS, seed)
    dp = [tuple(_pool_to_dev(t, head_major) for t in p) for p in pools]
    qd, knd, vnd = q.to(DEV), kn.to(DEV), vn.to(DEV)
    out = torch.empty_like(qd)
    full, stream = _classes(h, group, nf, ns, dp, knd, vnd)
    h.attn_decode_multi(qd, out, group, full, stream, SCALE)
    return out, ref, bud


# (group, T, nf, ns, lenA of the retrieval class, lenA of the streaming class, head-major pools)
PARITY_CASES = [
    (4, 2, 1, 1, 0, 0, True),           # segA empty: pure causal over the step's own rows
    (4, 4, 2, 6, 296, 381, True),       # a first decode step after a 296-row prefill, mixed layer
    (1, 16, 8, 0, 4083, 0, True),       # MHA: 16 tokens fill the columns; retrieval heads only, several splits
    (2, 8, 0, 8, 0, 384, True),         # streaming heads only
    (8, 2, 1, 1, 1, 383, True),         # a one-row pool
    (16, 2, 1, 1, 31, 0, True),         # one token per column block: two passes; the tile straddles A | B at row 31
    (4, 5, 2, 6, 39995, 380, True),     # ragged last column block, dozens of splits
    (4, 16, 1, 1, 4083, 384, True),     # four column blocks
    (1, 33, 1, 1, 267, 352, True),      # three column blocks; the causal triangle spans two 32-key tiles
    (4, 4, 1, 1, 29, 381, False),       # token-major pools; a tile straddles the A | B boundary
]


@pytest.mark.parametrize("group,T,nf,ns,lenF,lenS,head_major", PARITY_CASES)
def test_parity_with_the_oracle(group, T, nf, ns, lenF, lenS, head_major):
    out, ref, bud = _run(group, T, nf, ns, lenF, lenS, head_major)
    attn_close(out, ref, f"multi-token decode g{group} T{T} nf{nf} ns{ns} lenA {lenF}/{lenS} hm={head_major}", bud)


# ----------------------------------------------------------------------------- mask probe
@pytest.mark.parametrize("group,T", [(4, 2), (4, 4), (1, 16)])
@pytest.mark.parametrize("total", ["T", "31+T", 65, 300, 4099])
@pytest.mark.parametrize("as_stream", [False, True])
def test_mask_probe(group, T, total, as_stream):
    """q = 0 makes every visible key weigh 1 / n_vis; V of kv head i is one-hot at row j*_i (ones over the dims): token t's
    output for that head is 1 / n_vis(t) if it sees row j*_i and exactly 0.0 if not.  One kv head per probed row: both sides
    of every token's causal limit, row 0 and the last row."""
    h = _hip()
    L = {"T": T, "31+T": 31 + T}.get(total, total)
    lenA = L - T
    rows = sorted({0, L - 1} | {j for t in range(T) for j in (lenA + t, lenA + t + 1) if j < L})
    n_kv, Hq = len(rows), len(rows) * group
    g = torch.Generator().manual_seed(L * 64 + T)
    k = _rand((L, n_kv, D), g)
    v = torch.zeros(L, n_kv, D, dtype=torch.bfloat16)
    for i, j in enumerate(rows):
        v[j, i] = 1.0
    kd, vd = _pool_to_dev(k, True), _pool_to_dev(v, True)
    q = torch.zeros(T, Hq, D, dtype=torch.bfloat16, device=DEV)
    out = torch.full_like(q, float("nan"))
    segA = h.make_seg(kd[:lenA], vd[:lenA]) if lenA else h.make_seg(None, None)
    cls = h.make_class(n_kv, 0, segA, h.make_seg(kd[lenA:], vd[lenA:]))
    h.attn_decode_multi(q, out, group, None if as_stream else cls, cls if as_stream else None, SCALE)
    o = out.float().cpu().view(T, n_kv, group, D)
    for t in range(T):
        n_vis = lenA + t + 1
        want = 1.0 / n_vis
        ulp = 2.0 ** (math.floor(math.log2(want)) - 7)      # bf16: 8 significant bits
        for i, j in enumerate(rows):
            got = o[t, i]
            if j <= lenA + t:
                assert bool(((got - want).abs() <= ulp).all()), (t, j, float(got.min()), float(got.max()), want)
            else:
                assert bool((got == 0.0).all()), f"token {t} leaks row {j} (limit {lenA + t}): {float(got.abs().max())}"


# ----------------------------------------------------------------------------- dead rows and guard bytes
def _dead_case(group, T, nf, ns, lenF, lenS, head_major, B=None):
    """an entry point on identical live data with every byte outside the live regions zero, then poisoned: pools with 130
    dead rows behind their live length and gap heads around the class's heads, q / new rows with gaps between their tokens'
    heads, out inside a guard buffer.  B: the batched entry on B stacked cases."""
    h = _hip()
    cases = [_case(group, T, nf, ns, lenF, lenS, seed=50 + b) for b in range(B or 1)]
    stack = (lambda f: torch.stack([f(c) for c in cases])) if B else (lambda f: f(cases[0]))
    qb, kb, vb = (dead_embed(stack(lambda c, i=i: c[i]), lead=2, device=DEV) for i in range(3))
    pb = [[dead_embed(stack(lambda c, ci=ci, j=j: c[3][ci][j]), cap=L + 130, head_major=head_major, device=DEV) if n_h and L else None
           for j in range(2)] for ci, (n_h, L) in enumerate(((nf, lenF), (ns, lenS)))]
    ob = guard_embed(((B,) if B else ()) + (T, (nf + ns) * group, D), torch.bfloat16, device=DEV)
    bufs = [qb, kb, vb] + [t for p in pb for t in p if t is not None]
    zero = None
    for kind in ("zero",) + DEAD_KINDS:
        for b in bufs:
            b.reset(kind)
        ob.reset("guard")
        pools = [(p[0].live, p[1].live) if p[0] is not None else (None, None) for p in pb]
        cls = []
        for (lo, n_h), (pk, pv) in zip(((0, nf), (nf, ns)), pools):
            segA = h.make_seg(pk, pv) if pk is not None else h.make_seg(None, None)
            segB = h.make_seg(kb.view[..., lo:lo + n_h, :], vb.view[..., lo:lo + n_h, :])
            cls.append(h.make_class(n_h, lo * group, segA, segB) if n_h else None)
        (h.attn_decode_multi_batched if B else h.attn_decode_multi)(qb.view, ob.view, group, cls[0], cls[1], SCALE)
        got = _snap(ob.view)
        ob.assert_dead("guard", what=f"out ({kind})")
        for b in bufs:
            b.assert_dead(kind, what=f"inputs ({kind})")
        if zero is None:
            zero = got
            for b, c in enumerate(cases):       # two runs that agree cannot both be wrong (the budgeted bar; the noise ratio
                attn_close(ob.view[b] if B else ob.view, c[4], "", c[5].clone())        # is test_parity_with_the_oracle's)
        else:
            assert all(torch.equal(x, y) for x, y in zip(got, zero)), f"{kind}: output differs from the zero-filled run"


@pytest.mark.parametrize("head_major", [True, False])
@pytest.mark.parametrize("group,T,nf,ns,lenF,lenS", [(4, 5, 2, 1, 300, 29), (1, 16, 1, 1, 4083, 61), (8, 3, 1, 1, 0, 0)])
def test_dead_rows_and_guard_bytes(group, T, nf, ns, lenF, lenS, head_major):
    _dead_case(group, T, nf, ns, lenF, lenS, head_major)


def test_dead_rows_and_guard_bytes_batched():
    _dead_case(4, 5, 2, 1, 300, 29, True, B=2)


# ----------------------------------------------------------------------------- bit-equalities
def test_one_token_is_the_single_token_decode():
    h = _hip()
    group, nf, ns, lenF, lenS = 4, 2, 1, 5000, 29
    q, kn, vn, pools, _, _ = _case(group, 1, nf, ns, lenF, lenS)
    dp = [tuple(_pool_to_dev(t, True) for t in p) for p in pools]
    qd, knd, vnd = q.to(DEV), kn.to(DEV), vn.to(DEV)
    full, stream = _classes(h, group, nf, ns, dp, knd, vnd)
    a, b = torch.empty_like(qd), torch.empty_like(qd)
    h.attn_decode_multi(qd, a, group, full, stream, SCALE)
    h.attn_decode(qd[0], b[0], group, full, stream, SCALE)
    assert torch.equal(*_snap(a, b))


def test_batch_rows_equal_single_row_calls_and_runs_repeat():
    """B = 2 in one launch against two single-row calls, and the same call twice: bit for bit.  (Lengths at which the split
    plan is capped by the length's bucket — 16 and 1 splits — and not by the workgroup budget the batch rows share.)"""
    h = _hip()
    group, T, nf, ns, lenF, lenS, B = 4, 6, 2, 1, 4083, 29, 2
    cases = [_case(group, T, nf, ns, lenF, lenS, seed=70 + b) for b in range(B)]
    q, kn, vn = (torch.stack([c[i] for c in cases]).to(DEV) for i in range(3))
    pools = [tuple(torch.stack([c[3][ci][j] for c in cases]).transpose(1, 2).contiguous().to(DEV).transpose(1, 2) for j in range(2))
             for ci in range(2)]
    outs = [torch.empty_like(q) for _ in range(3)]
    for o in outs[:2]:
        full, stream = _classes(h, group, nf, ns, pools, kn, vn)
        h.attn_decode_multi_batched(q, o, group, full, stream, SCALE)
    for b in range(B):
        full, stream = _classes(h, group, nf, ns, [tuple(t[b] for t in p) for p in pools], kn[b], vn[b])
        h.attn_decode_multi(q[b], outs[2][b], group, full, stream, SCALE)
        attn_close(outs[2][b], cases[b][4], "", cases[b][5].clone())
    s = _snap(*outs)
    assert torch.equal(s[0], s[1]), "two runs of the same launch differ"
    assert torch.equal(s[0], s[2]), "batch rows differ from single-row calls"


# ----------------------------------------------------------------------------- the cache route
def test_cache_route(monkeypatch):
    """DuoAttentionStaticKVCache(multi_token_decode=True): after a 300-token prefill, steps of 5, 1, 16 and 17 tokens.  Every
    output is held to the oracle; pools and counters are bit-equal to a default cache fed the same inputs (RoPE, append and
    pool update are the launches they were); only the 5- and 16-token steps of the opted-in cache reach the new entry."""
    from duo_attn.backend import get_backend
    from duo_attn.patch import _duo
    from duo_attn.patch.static_kv_cache import DuoAttentionStaticKVCache
    from oracle.duo_oracle import StaticCacheRef, static_forward_ref

    assert _duo.MULTI_TOKEN_LIMIT == 16, "the steps below sit either side of the limit this test was written for"
    be = get_backend()
    calls = []
    inner = be.attention_multi
    monkeypatch.setattr(be, "attention_multi", lambda q, *a, **kw: (calls.append(q.shape[0]), inner(q, *a, **kw))[1], raising=False)
    L, Hq, Hkv, sink, recent = 2, 16, 4, 4, 28
    heads = heads_from_counts([1, 0], Hkv)
    steps = [300, 5, 1, 16, 17]
    total = sum(steps) + 8
    model = ShapeModel(L, Hq, Hkv, D, device=DEV)
    multi = DuoAttentionStaticKVCache(model, heads, 1, total, sink, recent, multi_token_decode=True)
    plain = DuoAttentionStaticKVCache(model, heads, 1, total, sink, recent)
    ref = StaticCacheRef(L, Hkv, D, heads, 1, total, sink, recent)
    g = torch.Generator().manual_seed(7)
    theta, pos = 500000.0, 0
    for S in steps:
        for l in range(L):
            q, k, v = _rand((1, S, Hq, D), g), _rand((1, S, Hkv, D), g), _rand((1, S, Hkv, D), g)
            n0 = len(calls)
            _duo.duo_static_attention_core(q.to(DEV), k.to(DEV), v.to(DEV), plain, l, pos, 1.0, theta)
            assert len(calls) == n0, "the default cache reached the multi-token entry"
            out = _duo.duo_static_attention_core(q.to(DEV), k.to(DEV), v.to(DEV), multi, l, pos, 1.0, theta)
            assert calls[n0:] == ([S] if S in (5, 16) else []), (S, calls[n0:])
            exp, bud = static_forward_ref(q, k, v, ref, l, pos, 1.0, theta, round_p=False, out_dtype=torch.float32,
                                          return_budget=True)
            attn_close(out, exp, f"multi-token cache route S={S} layer={l}", bud if S > 1 else None)
            assert multi.kv_seq_len_list == plain.kv_seq_len_list and multi.kv_seq_len_list[l] == ref.kv_seq_len_list[l]
            assert multi.streaming_kv_seq_len_list == plain.streaming_kv_seq_len_list
            for name in ("full_key_states_list", "full_value_states_list", "streaming_key_states_list", "streaming_value_states_list"):
                a, b = _snap(getattr(multi, name)[l], getattr(plain, name)[l])
                assert torch.equal(a, b), f"{name}[{l}] differs from the default cache after the {S}-token step"
            # keep the oracle on the device's pool contents so that later steps compare attention only
            n, m = ref.kv_seq_len_list[l], ref.streaming_kv_seq_len_list[l]
            ref.full_key_states_list[l][:, :n].copy_(multi.full_key_states_list[l][:, :n].cpu())
            ref.streaming_key_states_list[l][:, :m].copy_(multi.streaming_key_states_list[l][:, :m].cpu())
        pos += S
