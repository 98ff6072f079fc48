"""CPU: the multi-token INT4 decode entry points exist at every layer — declared in the header, typed in the ctypes binding,
exported by the built library — and the cache constructor takes the opt-in flag.  Argument errors are host-side."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("duo_attn_decode_int4_multi_f16", "duo_attn_decode_int4_multi_batched_f16")


def test_header_binding_and_library_agree_on_the_new_entry_points():
    from duo_attn import _hip

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "duo_attn_hip.h")).read(), flags=re.S)
    lib = _hip.load_library()
    for name in NAMES:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", hdr)
        assert proto, f"{name} not declared"
        assert len(proto.group(1).split(",")) == len(_hip._SIGNATURES[name][1]), name
        assert name in _hip.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _hip.ABI_VERSION == lib.duo_abi_version() == 8
    assert callable(_hip.attn_decode_int4_multi) and callable(_hip.attn_decode_int4_multi_batched)


def test_argument_errors_are_host_side():
    from duo_attn import _hip

    lib = _hip.load_library()
    f = lib.duo_attn_decode_int4_multi_f16
    assert f(None, 0, 0, None, 0, 0, 2, 4, None, None, 1.0, 128, 0, None, 0, None) == -1       # null q
    assert f(None, 0, 0, None, 0, 0, 2, 4, None, None, 1.0, 64, 0, None, 0, None) == -2        # head_dim
    import ctypes

    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert f(p, 512, 128, p, 512, 128, 0, 4, None, None, 1.0, 128, 0, None, 0, None) == -1     # n_tokens < 1
    assert f(p, 512, 128, p, 512, 128, 65, 4, None, None, 1.0, 128, 0, None, 0, None) == -1    # n_tokens > 64
    assert f(p, 512, 128, p, 512, 128, 2, 17, None, None, 1.0, 128, 0, None, 0, None) == -3    # group > 16: DUO_EGROUP
    pool = _hip.Int4Pool()
    pool.k_q = pool.v_q = pool.k_sz = pool.v_sz = p.value
    pool.len, pool.n_kv_heads = 3, 1
    assert f(p, 512, 128, p, 512, 128, 4, 4, ctypes.byref(pool), None, 1.0, 128, 0, None, 0, None) == -1   # len < n_tokens


def test_cache_constructor_takes_the_flag():
    from duo_attn.int4_kv import DuoAttentionStaticINT4KVCache
    from duo_attn.patch import int4

    params = inspect.signature(DuoAttentionStaticINT4KVCache.__init__).parameters
    assert params["multi_token_decode"].default is False
    assert callable(DuoAttentionStaticINT4KVCache.multi_token_attention)
    assert 1 < int4.MULTI_TOKEN_LIMIT <= 64
