"""GPU: the tiny fp16 Llama of tests/test_int4_model_gpu.py through the INT4 dual cache with and without
``multi_token_decode``: a prefill, then steps of 4, 1 and 2 tokens.  The flag only changes which kernels compute the
attention of the multi-token steps (the packed-pool kernel instead of get() + the fp16 prefill kernel), so the logits of the
two runs agree within the bar that file's ``_close16`` applies to attention outputs against the oracle, and only the flagged
run calls the new entry point.

``_close16`` is 1e-3 |ref| + 2^-10 |ref| + 2^-10 budget + 1e-3 rms(ref), where for an attention output sum_j p_j v_j the budget is
sum_j p_j |v_j|: the size of the output's error when every term carries a relative error of one fp16 rounding.  The logits are
sum_j W_ij h_j of the LM head over the final normed hidden state h, so their budget in the same sense is sum_j |W_ij| |h_j|: the
two routes hand the following fp16 linears attention outputs that differ by such roundings (each meets ``_close16`` against the
oracle, tests/test_int4_multi_gpu.py), and h differs between the runs by fp16 roundings of its elements.  The budget is taken
from the unflagged run (the reference of the comparison)."""
import copy

import pytest
import torch

from test_int4_model_gpu import DEV, HEADS, _close16, tiny16

pytestmark = pytest.mark.gpu


def test_model_multi_token_steps_match_the_prefill_route(monkeypatch):
    from duo_attn import _hip
    from duo_attn.int4_kv import DuoAttentionStaticINT4KVCache
    from duo_attn.patch.int4 import enable_duo_attention_int4_kv_eval

    calls = []
    real = _hip.attn_decode_int4_multi_batched

    def counted(q, *a, **kw):
        calls.append(tuple(q.shape))
        return real(q, *a, **kw)

    monkeypatch.setattr(_hip, "attn_decode_int4_multi_batched", counted)
    model = copy.deepcopy(tiny16(seed=31))
    enable_duo_attention_int4_kv_eval(model, HEADS.copy())
    steps = [64, 37, 4, 1, 2]
    N = sum(steps)
    ids = torch.randint(0, 211, (1, N), generator=torch.Generator().manual_seed(32)).to(DEV)
    logits, n_calls, head_in = {}, {}, {}
    grab = []
    hook = model.lm_head.register_forward_hook(lambda mod, args, out: grab.append(args[0].detach().float().cpu()))
    for flag in (False, True):
        del calls[:]
        kv = DuoAttentionStaticINT4KVCache(model, HEADS, 1, N + 8, 8, 24, 64, multi_token_decode=flag)
        pos, got = 0, []
        with torch.no_grad():
            for c in steps:
                got.append(model(input_ids=ids[:, pos:pos + c], past_key_values=kv, use_cache=True).logits.float().cpu())
                pos += c
        assert kv.kv_seq_len == N and kv.streaming_kv_seq_len_list[0] == 8 + 24
        logits[flag], n_calls[flag], head_in[flag] = got, list(calls), list(grab)
        del grab[:]
    hook.remove()
    w_abs = model.lm_head.weight.detach().float().cpu().abs()
    # three layers x the steps of 4 and 2 tokens; the 37-token chunk and the single token keep their routes
    assert n_calls[False] == []
    assert n_calls[True] == [(1, 4, 4, 128)] * 3 + [(1, 2, 4, 128)] * 3
    for i, (c, a, b) in enumerate(zip(steps, logits[True], logits[False])):
        assert torch.isfinite(a).all()
        if i < 2:
            assert torch.equal(a, b), c          # before the first multi-token step the two runs are the same launches
        bud = head_in[False][i].abs() @ w_abs.T         # sum_j |W_ij| |h_j| of the reference run's LM head
        assert bud.shape == b.shape
        err = (a - b).abs()
        tol = 1e-3 * b.abs() + 2.0 ** -10 * b.abs() + 2.0 ** -10 * bud + 1e-3 * b.pow(2).mean().sqrt()
        print(f"step of {c}: max err {err.max():.3e}, worst err / tol {float((err / tol).max()):.3f}, "
              f"budget term {float(2.0 ** -10 * bud.mean()):.3e}, rms term {float(1e-3 * b.pow(2).mean().sqrt()):.3e}")
        _close16(a, b, bud, f"step of {c}")
