"""CPU: the bf16 multi-token decode step exists at every layer — declared in the header, typed in the ctypes binding, exported
by the built library, routed by duo_static_attention_core behind the cache's opt-in flag — and its argument errors are
host-side (no device, no launch)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from helpers import ShapeModel, heads_from_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("duo_attn_decode_multi_workspace_bytes", "duo_attn_decode_multi_bf16", "duo_attn_decode_multi_batched_bf16")
C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}


def _ctype(decl, hip):
    """the ctypes type of one C parameter / return declaration of the header"""
    decl = decl.replace("const", "").strip()
    if "duo_head_class" in decl:
        return ctypes.POINTER(hip.HeadClass)
    if "*" in decl:
        return ctypes.c_void_p
    return C_TYPES[decl.split()[0]]


def test_header_declarations_equal_the_binding():
    from duo_attn import _hip

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "duo_attn_hip.h")).read(), flags=re.S)
    lib = _hip.load_library()
    for name in NAMES:
        proto = re.search(r"\b(int64_t|int)\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert proto, f"{name} not declared"
        restype, argtypes = _hip._SIGNATURES[name]
        assert restype is _ctype(proto.group(1), _hip), name
        got = [_ctype(a, _hip) for a in proto.group(2).split(",")]
        assert got == list(argtypes), (name, got, argtypes)
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert callable(_hip.attn_decode_multi) and callable(_hip.attn_decode_multi_batched)


def test_abi_version_is_unchanged():
    from duo_attn import _hip

    assert _hip.load_library().duo_abi_version() == _hip.ABI_VERSION == 8


def _class(hip, p, n_kv, lenA, lenB, token_stride=128, head_stride=128 * 512):
    c = hip.HeadClass()
    c.n_kv_heads, c.q_head_offset = n_kv, 0
    for seg, n in ((c.segA, lenA), (c.segB, lenB)):
        seg.k = seg.v = p.value if n else None
        seg.token_stride, seg.head_stride, seg.len, seg.batch_stride = token_stride, head_stride, n, 0
    return c


def test_argument_errors_are_host_side():
    """every refusal comes back before any launch: the pointers here are host memory and no device is needed"""
    from duo_attn import _hip

    lib = _hip.load_library()
    f, fb = lib.duo_attn_decode_multi_bf16, lib.duo_attn_decode_multi_batched_bf16
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = _class(_hip, p, 2, 300, 4)
    big = 1 << 30

    def call(n_tokens=4, group=4, cls=ok, head_dim=128, ws=p, ws_bytes=big, q=p):
        return f(q, 2048, 128, p, 2048, 128, n_tokens, group, ctypes.byref(cls), None, 1.0, head_dim, ws, ws_bytes, None)

    assert call(q=None) == -1                                   # null q
    assert call(n_tokens=0) == -1 and call(n_tokens=65) == -1   # 1 <= n_tokens <= 64
    assert call(head_dim=64) == -2                              # DUO_EHEADDIM
    assert call(group=3) == -3 and call(group=32) == -3         # DUO_EGROUP: 1, 2, 4, 8, 16 only
    assert call(cls=_class(_hip, p, 2, 300, 3)) == -1           # segB.len != n_tokens
    assert call(cls=_class(_hip, p, 2, 300, 5)) == -1
    assert call(cls=_class(_hip, p, 2, 300, 4, token_stride=132)) == -1     # rows not 16-byte aligned
    assert fb(p, 0, 2048, 128, p, 0, 2048, 128, -1, 4, 4, ctypes.byref(ok), None, 1.0, 128, p, big, None) == -1
    # workspace: 40000 rows of 2 kv heads plan 64 splits (bucket 1024 / 8 caps 128; 256 workgroups / 2 heads / 2 column blocks)
    long = _class(_hip, p, 2, 40000 - 5, 5)
    need = lib.duo_attn_decode_multi_workspace_bytes(8, 5, 64)
    assert need == 5 * 8 * 64 * 130 * 4
    if not os.environ.get("DUO_DECODE_TARGET_WGS") and not os.environ.get("DUO_DECODE_SPLIT_DIV"):
        assert call(n_tokens=5, cls=long, ws_bytes=need - 1) == -4      # one byte short: DUO_EWORKSPC
        assert call(n_tokens=5, cls=long, ws=None, ws_bytes=0) == -4


def test_workspace_bytes_is_monotone():
    from duo_attn import _hip

    w = _hip.load_library().duo_attn_decode_multi_workspace_bytes
    assert w(0, 4, 4) == w(8, 0, 4) == w(8, 4, 0) == 0
    by_t = [w(32, t, 16) for t in range(1, 65)]
    by_s = [w(32, 8, s) for s in range(1, 129)]
    assert all(a < b for a, b in zip(by_t, by_t[1:])) and all(a < b for a, b in zip(by_s, by_s[1:]))
    assert w(32, 1, 16) == _hip.load_library().duo_attn_decode_workspace_bytes(32, 16)


def test_cache_constructor_takes_the_flag_as_a_trailing_keyword():
    from duo_attn.patch import _duo
    from duo_attn.patch.static_kv_cache import DuoAttentionStaticKVCache

    # the reference's positional signature stays what introspection reports
    assert list(inspect.signature(DuoAttentionStaticKVCache.__init__).parameters)[1:] == [
        "model", "full_attention_heads", "batch_size", "max_size", "sink_size", "recent_size"]
    heads = heads_from_counts([1], 2)
    assert DuoAttentionStaticKVCache(ShapeModel(1, 4, 2), heads, 1, 8, 2, 2).multi_token_decode is False
    assert DuoAttentionStaticKVCache(ShapeModel(1, 4, 2), heads, 1, 8, 2, 2, multi_token_decode=True).multi_token_decode is True
    with pytest.raises(TypeError):
        DuoAttentionStaticKVCache(ShapeModel(1, 4, 2), heads, 1, 8, 2, 2, True)      # keyword-only
    assert 1 <= _duo.MULTI_TOKEN_LIMIT <= 64


def _recording_backend():
    from oracle.duo_oracle import OracleBackend

    class Recording(OracleBackend):
        """the oracle, noting which attention entry a step went to (both compute the same thing)"""

        def __init__(self):
            super().__init__()
            self.calls = []

        def attention(self, q, out, group, full, stream, scale):
            self.calls.append(("attention", q.shape[0]))
            super().attention(q, out, group, full, stream, scale)

        def attention_multi(self, q, out, group, full, stream, scale):
            self.calls.append(("attention_multi", q.shape[0]))
            super().attention(q, out, group, full, stream, scale)

    return Recording()


@pytest.mark.parametrize("flag", [False, True])
def test_routing_predicate(flag):
    """only a step with the flag set, a non-empty past and 1 < T <= MULTI_TOKEN_LIMIT changes its attention call; the first
    chunk, one-token steps, longer steps and every step of a default cache keep theirs"""
    from duo_attn import backend
    from duo_attn.patch import _duo
    from duo_attn.patch.static_kv_cache import DuoAttentionStaticKVCache

    lim = _duo.MULTI_TOKEN_LIMIT
    Hq, Hkv, D = 8, 2, 128
    heads = heads_from_counts([1, 0], Hkv)
    steps = [6, 1, 2, lim, lim + 1] if lim > 1 else [6, 1, 2]
    rec = _recording_backend()
    backend._set_backend_for_testing(rec)
    try:
        cache = DuoAttentionStaticKVCache(ShapeModel(2, Hq, Hkv, D), heads, 1, 64 + sum(steps), 2, 4, multi_token_decode=flag)
        assert cache.multi_token_decode is flag
        g = torch.Generator().manual_seed(0)
        pos = 0
        for S in steps:
            for l in range(2):
                q, k, v = (torch.randn(1, S, h, D, generator=g).to(torch.bfloat16) for h in (Hq, Hkv, Hkv))
                _duo.duo_static_attention_core(q, k, v, cache, l, pos, 1.0, 10000.0)
            pos += S
    finally:
        backend._set_backend_for_testing(None)
    want = [("attention_multi" if flag and i > 0 and 1 < S <= lim else "attention", S) for i, S in enumerate(steps) for _ in range(2)]
    assert rec.calls == want
    # a float16 step and an unsupported group stay on their current call whatever the flag says
    assert not _duo.multi_token_route(cache, 10, 4, torch.float16, 4)
    assert not _duo.multi_token_route(cache, 10, 4, torch.bfloat16, 3)
    assert _duo.multi_token_route(cache, 10, 2, torch.bfloat16, 4) is (flag and lim >= 2)
