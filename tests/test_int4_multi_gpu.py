"""GPU: a step of T > 1 query tokens against non-empty INT4 pools, computed on the packed pools
(duo_attn_decode_int4_multi[_batched]_f16; reference demo/w8a8kv4_llama.py:239-274 after put(), before compress()):
token i of a head attends to rows [0, len - T + i] of its class's dequantised pool, bottom-right causal.

Parity against exact fp32 softmax attention over the oracle's dequantised rows at the single-token decode bar of
tests/test_int4.py::test_fused_int4_decode (rms taken per token, as that test's one token has it), an exact probe of the
causal mask, bit-level consistency with the single-token entry point / across modes / across batch rows, and the cache
object's route against its prefill_attention twin."""
import numpy as np
import pytest
import torch

from helpers import ShapeModel, heads_from_counts
from oracle.int4_oracle import dequantize_int4_ref, quantize_int4_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCALE = 128 ** -0.5


def _pools(T, h, head_major=True, batch=None):
    lead = () if batch is None else (batch,)
    if head_major:
        perm = (1, 0, 2) if batch is None else (0, 2, 1, 3)
        q = torch.zeros(*lead, h, T, 64, dtype=torch.uint8, device=DEV).permute(*perm)
        sz = torch.zeros(*lead, h, T, 2, dtype=torch.float16, device=DEV).permute(*perm)
    else:
        q = torch.zeros(*lead, T, h, 64, dtype=torch.uint8, device=DEV)
        sz = torch.zeros(*lead, T, h, 2, dtype=torch.float16, device=DEV)
    return q, sz


def _dq(x, fused=False):
    """[rows, h, 128] fp16 tensor -> what the pool holds of it, dequantised by the oracle in the form `fused` selects, fp32"""
    return torch.from_numpy(dequantize_int4_ref(*quantize_int4_ref(x.float().numpy()), fused=bool(fused)).astype(np.float32))


def _make_pool(k, v, off, head_major=True, spare=3):
    """quantise k / v [rows, h, 128] fp16 into fresh pools -> Int4Pool over all the rows"""
    from duo_attn import _hip

    T, h = k.shape[0], k.shape[1]
    kq, ksz = _pools(T + spare, h, head_major)
    vq, vsz = _pools(T + spare, h, head_major)
    _hip.int4_quantize(k.to(DEV), kq, ksz, 0)
    _hip.int4_quantize(v.to(DEV), vq, vsz, 0)
    p = _hip.make_int4_pool(kq, ksz, vq, vsz, T, off)
    p._keep = (kq, ksz, vq, vsz)
    return p


def _ref_multi(q, kd, vd, group):
    """q [T, Hq, 128] fp32, kd / vd [L, h, 128] fp32 (dequantised) -> exact attention [T, Hq, 128] fp32 with token i over rows
    [0, L - T + i], and the budget sum_j p_j |v_j|"""
    T, Hq, L = q.shape[0], q.shape[1], kd.shape[0]
    out, bud = torch.empty(T, Hq, 128), torch.empty(T, Hq, 128)
    vis = torch.arange(L)[None, :] <= (L - T + torch.arange(T))[:, None]
    for hq in range(Hq):
        k, v = kd[:, hq // group], vd[:, hq // group]
        s = (q[:, hq] @ k.T) / (128 ** 0.5)
        p = torch.softmax(s.masked_fill(~vis, float("-inf")), 1)
        out[:, hq] = p @ v
        bud[:, hq] = p @ v.abs()
    return out, bud


def _bar(ref, bud):
    """the bar of test_fused_int4_decode, element by element; rms(ref) per token ([Hq, 128] slab, what that test's ref is)"""
    rms = ref.pow(2).mean(dim=(-2, -1), keepdim=True).sqrt()
    return 1e-3 * ref.abs() + 2.0 ** -10 * ref.abs() + 2.0 ** -10 * bud + 1e-3 * rms


def _rand_kv(g, rows, h, odd_rows):
    k = torch.randn(rows, h, 128, generator=g)
    v = torch.randn(rows, h, 128, generator=g)
    if odd_rows:        # scales outside [2^-10, 64): the tile's vote takes the general dequantisation (as test_int4.py)
        for x, big in ((k, 300.0), (v, 800.0)):
            f = torch.ones(rows, h, 1)
            u = torch.rand(rows, h, 1, generator=g)
            f[u < 0.1] = 1e-3
            f[u > 0.995] = big
            x *= f
    return k.to(torch.float16), v.to(torch.float16)


# (group, T, nf, ns, n_full, n_stream, odd_rows, fused, head_major); n_full / n_stream given relative to T where the issue
# does: T (pure causal), T + 1, 384 + T.  One pass exactly full: (4, 4) (1, 16) (2, 8) (8, 2); partly full: (4, 2); two and four
# passes: (16, 2) (4, 5) (4, 16); ragged last pass: (4, 5) (1, 33).
CASES = [
    (4, 2, 1, 1, 2, 2, False, 0, True),
    (4, 4, 2, 6, 300, 385, True, 1, True),
    (1, 16, 8, 0, 4099, 0, False, 0, True),
    (2, 8, 0, 8, 0, 384 + 8, True, 0, True),
    (8, 2, 1, 1, 3, 385, False, 1, True),
    (16, 2, 1, 1, 33, 2, True, 0, True),
    (4, 5, 2, 6, 40000, 385, True, 0, True),
    (4, 16, 1, 1, 4099, 384 + 16, False, 1, True),
    (1, 33, 1, 1, 300, 385, True, 0, True),
    (4, 4, 1, 1, 33, 385, False, 0, False),
    (4, 16, 1, 1, 16, 17, True, 0, True),
    (2, 8, 2, 6, 40000, 8, False, 1, True),
]


@pytest.mark.parametrize("group,T,nf,ns,n_full,n_stream,odd_rows,fused,head_major", CASES)
def test_multi_token_parity(group, T, nf, ns, n_full, n_stream, odd_rows, fused, head_major):
    from duo_attn import _hip

    g = torch.Generator().manual_seed(1000 * T + n_full + n_stream)
    Hq = (nf + ns) * group
    q = torch.randn(T, Hq, 128, generator=g).to(torch.float16)
    ref, bud = torch.empty(T, Hq, 128), torch.empty(T, Hq, 128)
    pools = []
    for n_h, rows, off in ((nf, n_full, 0), (ns, n_stream, nf * group)):
        if n_h == 0:
            pools.append(None)
            continue
        k, v = _rand_kv(g, rows, n_h, odd_rows)
        pools.append(_make_pool(k, v, off, head_major))
        sl = slice(off, off + n_h * group)
        ref[:, sl], bud[:, sl] = _ref_multi(q.float()[:, sl], _dq(k, fused), _dq(v, fused), group)
    out = torch.full((T, Hq, 128), float("nan"), dtype=torch.float16, device=DEV)
    _hip.attn_decode_int4_multi(q.to(DEV), out, group, pools[0], pools[1], SCALE, fused=fused)
    o = out.float().cpu()
    assert torch.isfinite(o).all()
    err, tol = (o - ref).abs(), _bar(ref, bud)
    worst = float((err / tol.clamp_min(1e-30)).max())
    print(f"multi parity G={group} T={T} n={n_full}/{n_stream}: max err {err.max():.3e}, worst err / tol {worst:.3f}")
    assert (err <= tol).all(), f"max err {err.max():.3e}, worst err / tol {worst:.3f}"


@pytest.mark.parametrize("group,T", [(4, 2), (4, 4), (1, 16)])
@pytest.mark.parametrize("length", ["T", "31+T", 65, 300, 4099])
def test_multi_token_mask_is_exact(group, T, length):
    """q = 0: every visible key weighs the same.  V row j* = 1.0 (constant rows quantise exactly), every other row 0: token i's
    output is 1 / (len - T + i + 1) if j* <= len - T + i and exactly 0.0 otherwise.  One kv head per j*: both sides of every
    token's limit, row 0, the last row.  (4099: several splits, beyond the lengths the issue lists.)"""
    from duo_attn import _hip

    L = {"T": T, "31+T": 31 + T}.get(length, length)
    stars = sorted({0, L - 1} | {j for i in range(T) for j in (L - T + i, L - T + i + 1) if j < L})
    h = len(stars)
    g = torch.Generator().manual_seed(L)
    k = torch.randn(L, h, 128, generator=g).to(torch.float16)
    v = torch.zeros(L, h, 128, dtype=torch.float16)
    for kv, j in enumerate(stars):
        v[j, kv] = 1.0
    pool = _make_pool(k, v, 0)
    q = torch.zeros(T, h * group, 128, dtype=torch.float16, device=DEV)
    for fused in (0, 1):
        out = torch.full((T, h * group, 128), float("nan"), dtype=torch.float16, device=DEV)
        _hip.attn_decode_int4_multi(q, out, group, pool, None, SCALE, fused=fused)
        o = out.float().cpu()
        for i in range(T):
            n_vis = L - T + i + 1
            want = torch.tensor(1.0 / n_vis, dtype=torch.float16).float()
            ulp = 2.0 ** (np.floor(np.log2(float(want))) - 10)
            for kv, j in enumerate(stars):
                got = o[i, kv * group:(kv + 1) * group]
                if j <= L - T + i:
                    assert ((got - want).abs() <= ulp).all(), (fused, i, j, float(got.min()), float(got.max()), float(want))
                else:
                    assert (got == 0.0).all(), (fused, i, j, float(got.abs().max()))


def _two_class(g, group, T, n_full, n_stream, nf=1, ns=1):
    Hq = (nf + ns) * group
    q = torch.randn(T, Hq, 128, generator=g).to(torch.float16).to(DEV)
    full = _make_pool(*_rand_kv(g, n_full, nf, True), 0)
    stream = _make_pool(*_rand_kv(g, n_stream, ns, True), nf * group)
    return q, full, stream


def test_one_token_equals_single_token_entry():
    from duo_attn import _hip

    q, full, stream = _two_class(torch.Generator().manual_seed(1), 4, 1, 4099, 385)
    for fused in (0, 1, 2):
        a, b = torch.zeros_like(q), torch.zeros_like(q)
        _hip.attn_decode_int4_multi(q, a, 4, full, stream, SCALE, fused=fused)
        _hip.attn_decode_int4(q[0], b[0], 4, full, stream, SCALE, fused=fused)
        assert torch.equal(a, b), fused


def test_folded_modes_run_the_dequantising_form():
    from duo_attn import _hip

    q, full, stream = _two_class(torch.Generator().manual_seed(2), 4, 5, 4099, 385)
    outs = []
    for fused in (0, 1, 2, 3):
        o = torch.zeros_like(q)
        _hip.attn_decode_int4_multi(q, o, 4, full, stream, SCALE, fused=fused)
        outs.append(o)
    assert torch.equal(outs[2], outs[0]) and torch.equal(outs[3], outs[1])
    assert not torch.equal(outs[0], outs[1])        # (the two dequantisation forms do differ on this data)


@pytest.mark.parametrize("padded_out", [False, True])
def test_batch_rows_equal_single_rows(padded_out):
    """B = 2 rows with different data in one launch pair == each row alone (4099 rows: 16 splits and the merge either way;
    padded_out: batch rows of `out` not T token strides apart — the merge then runs once per batch row)"""
    from duo_attn import _hip

    group, T, nf, ns, n_full, n_stream, B = 4, 5, 1, 1, 4099, 385, 2
    g = torch.Generator().manual_seed(3)
    Hq = (nf + ns) * group
    q = torch.randn(B, T, Hq, 128, generator=g).to(torch.float16).to(DEV)
    bufs = []
    for n_h, rows in ((nf, n_full), (ns, n_stream)):
        kq, ksz = _pools(rows + 3, n_h, batch=B)
        vq, vsz = _pools(rows + 3, n_h, batch=B)
        for b in range(B):
            k, v = _rand_kv(g, rows, n_h, True)
            _hip.int4_quantize(k.to(DEV), kq[b], ksz[b], 0)
            _hip.int4_quantize(v.to(DEV), vq[b], vsz[b], 0)
        bufs.append((kq, ksz, vq, vsz))
    full = _hip.make_int4_pool(*bufs[0], n_full, 0)
    stream = _hip.make_int4_pool(*bufs[1], n_stream, nf * group)
    out = torch.full((B, T + int(padded_out), Hq, 128), float("nan"), dtype=torch.float16, device=DEV)[:, :T]
    _hip.attn_decode_int4_multi_batched(q, out, group, full, stream, SCALE)
    for b in range(B):
        f1 = _hip.make_int4_pool(*(t[b] for t in bufs[0]), n_full, 0)
        s1 = _hip.make_int4_pool(*(t[b] for t in bufs[1]), n_stream, nf * group)
        solo = torch.zeros(T, Hq, 128, dtype=torch.float16, device=DEV)
        _hip.attn_decode_int4_multi(q[b], solo, group, f1, s1, SCALE)
        assert torch.isfinite(out[b].float()).all() and torch.equal(out[b], solo), b
    assert not torch.equal(out[0], out[1])


def test_argument_errors():
    from duo_attn import _hip

    g = torch.Generator().manual_seed(4)
    q, full, stream = _two_class(g, 4, 5, 300, 4)           # streaming pool shorter than the step
    with pytest.raises(_hip.DuoHipError):
        _hip.attn_decode_int4_multi(q, torch.zeros_like(q), 4, full, stream, SCALE)
    q, full, stream = _two_class(g, 4, 65, 300, 300)        # more tokens than one call takes
    with pytest.raises(_hip.DuoHipError):
        _hip.attn_decode_int4_multi(q, torch.zeros_like(q), 4, full, stream, SCALE)
    torch.cuda.synchronize()


def test_cache_multi_token_route_matches_prefill_twin():
    """DuoAttentionStaticINT4KVCache(multi_token_decode=True).multi_token_attention against prefill_attention of a twin
    without the flag, on the same inputs: chunked put / compress, then steps of 3, 1 and 4 tokens with the streaming pool
    already at sink + recent.  Both against the oracle restatement of test_int4_cache_chunked_prefill_attention (the new route
    at the fp16 decode bar, the twin at the bar that test holds it to); pools and counters identical afterwards."""
    from duo_attn.int4_kv import DuoAttentionStaticINT4KVCache
    from helpers import attn_close

    counts, Hq, Hkv, sink, recent, chunk = [1, 3, 0, 4], 16, 4, 16, 48, 200
    G, W = Hq // Hkv, sink + recent
    model = ShapeModel(len(counts), Hq, Hkv, 128, device=DEV, dtype=torch.float16)
    heads = heads_from_counts(counts, Hkv)
    new = DuoAttentionStaticINT4KVCache(model, heads, 1, 700, sink, recent, chunk, multi_token_decode=True)
    twin = DuoAttentionStaticINT4KVCache(model, heads, 1, 700, sink, recent, chunk)
    assert new.multi_token_decode and not twin.multi_token_decode
    g = torch.Generator().manual_seed(6)
    hist = [dict(fk=torch.zeros(0, nf, 128), fv=torch.zeros(0, nf, 128), sk=torch.zeros(0, Hkv - nf, 128),
                 sv=torch.zeros(0, Hkv - nf, 128)) for nf in counts]
    for S in (200, 150, 3, 1, 4):
        for l, nf in enumerate(counts):
            q = torch.randn(1, S, Hq, 128, generator=g).to(torch.float16)
            k = torch.randn(1, S, Hkv, 128, generator=g).to(torch.float16)
            v = torch.randn(1, S, Hkv, 128, generator=g).to(torch.float16)
            for c in (new, twin):
                c.put(l, k.to(DEV), v.to(DEV), dequantize=False)
            h = hist[l]
            h["fk"], h["fv"] = torch.cat([h["fk"], _dq(k[0, :, :nf])]), torch.cat([h["fv"], _dq(v[0, :, :nf])])
            h["sk"], h["sv"] = torch.cat([h["sk"], _dq(k[0, :, nf:])]), torch.cat([h["sv"], _dq(v[0, :, nf:])])
            if S <= 4:
                if Hkv - nf:
                    assert new.streaming_kv_seq_len_list[l] == W + S      # the window was full before this step
                ref, bud = torch.empty(S, Hq, 128), torch.empty(S, Hq, 128)
                if nf:
                    ref[:, :nf * G], bud[:, :nf * G] = _ref_multi(q[0, :, :nf * G].float(), h["fk"], h["fv"], G)
                if Hkv - nf:
                    ref[:, nf * G:], bud[:, nf * G:] = _ref_multi(q[0, :, nf * G:].float(), h["sk"], h["sv"], G)
                if S == 1:
                    a, b = new.decode_attention(l, q.to(DEV)), twin.decode_attention(l, q.to(DEV))
                    assert torch.equal(a, b)
                else:
                    a = new.multi_token_attention(l, q.to(DEV))
                    b = twin.prefill_attention(l, q.to(DEV), k.to(DEV), v.to(DEV))
                    attn_close(b[0], ref, f"twin prefill_attention S={S} layer {l}", bud)
                err, tol = (a[0].float().cpu() - ref).abs(), _bar(ref, bud)
                assert torch.isfinite(a.float()).all() and (err <= tol).all(), (S, l, float(err.max()))
            for c in (new, twin):
                c.compress(l)
            if h["sk"].shape[0] > W:
                h["sk"] = torch.cat([h["sk"][:sink], h["sk"][-recent:]])
                h["sv"] = torch.cat([h["sv"][:sink], h["sv"][-recent:]])
    assert new.kv_seq_len_list == twin.kv_seq_len_list and new.streaming_kv_seq_len_list == twin.streaming_kv_seq_len_list
    for name in ("full_key_caches", "full_value_caches", "streaming_key_caches", "streaming_value_caches"):
        for ca, cb in zip(getattr(new, name), getattr(twin, name)):
            assert torch.equal(ca.quantized_data, cb.quantized_data) and torch.equal(ca.scale_zero, cb.scale_zero), name
